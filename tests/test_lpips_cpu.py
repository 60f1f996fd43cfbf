"""CPU tier (-m "not gpu"): the host-only half of the LPIPS row -- the C ABI of the ``dfh_lpips_*`` family in all three
places (header, both libraries, ctypes), the 33-entry parameter table, the packed / workspace size formulas, every host guard with
made-up addresses, the Python class's refusals and its three weight routes, the plain-torch restatement against the fixtures, and a
sanitizer run of the table, plan and guards as a stand-alone program.  No compute call is made here; the kernels are held to the same
fixtures on the GPU (tests/test_gpu_lpips.py)."""
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
from difashion_amd.lpips import im2tensor_table
from tests import helpers_lpips as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_lpips_create", "dfh_lpips_destroy", "dfh_lpips_num_params", "dfh_lpips_param_name", "dfh_lpips_param_ndim", "dfh_lpips_param_dim",
          "dfh_lpips_packed_bytes", "dfh_lpips_pack", "dfh_lpips_workspace_bytes", "dfh_lpips_forward", "dfh_lpips_group_argmin", "dfh_lpips_prep",
          "dfh_lpips_conv3x3_relu", "dfh_lpips_maxpool2x2", "dfh_lpips_layer_score"]
PACKED_BYTES = 4 * sum(9 * ((w[1] + 3) // 4 * 4) * w[0] for n, w in H.param_shapes().items() if n.startswith("net.") and n.endswith(".weight"))


def workspace_bytes(pairs, h, w):
    """The formula include/difashion_hip.h states: two ping-pong buffers of 2 pairs images x H x W x 64 floats, 5 x 256 partial sums a pair."""
    return 4 * (2 * (2 * pairs * h * w * 64) + pairs * 5 * 256) + 256


@pytest.fixture()
def ctx():
    h = C.c_void_p()
    _lib.call("dfh_lpips_create", C.byref(_lib.LpipsConfigC(0)), C.byref(h))
    yield h
    _lib.raw().dfh_lpips_destroy(h)


def test_every_lpips_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dfh_lpips_[a-z0-9_]+)\s*\(", src)) == set(FAMILY)
    assert "#define DFH_ABI_VERSION 8" in src and "#define DFH_LPIPS_NUM_PARAMS 33" in src
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds export the row
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY:
        assert n in _lib.SIGNATURES, n
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "lpips.hip" in mk and re.search(r"lpips\.o:.*\n\t.*-ffp-contract=off", mk)
    text = open(os.path.join(_lib.CSRC, "lpips.hip")).read()
    # one source for both builds, fp32 only, no atomics, nothing allocated
    assert not re.search(r"\b(bf16_t|h16x8_t|DFH_F16|pack2bf|f2bf|atomic[A-Z]\w*|__hip_atomic\w*|getenv|hipMalloc\w*)\b", text)


def test_parameter_table_is_the_packages_state_dict(ctx):
    m = da.LPIPS(init_seed=None)
    table = m.param_table()
    assert len(table) == 33 == _lib.raw().dfh_lpips_num_params(ctx)
    assert table == [(k, tuple(v)) for k, v in H.param_shapes().items()]
    assert [n for n, _ in table[:3]] == ["scaling_layer.shift", "scaling_layer.scale", "net.slice1.0.weight"]
    assert table[2][1] == (64, 3, 3, 3) and table[-1] == ("lin4.model.1.weight", (1, 512, 1, 1)) and table[26] == ("net.slice5.28.weight", (512, 512, 3, 3))
    sd = m.state_dict()
    assert list(sd) == [n for n, _ in table] and all(tuple(sd[n].shape) == s for n, s in table)
    assert torch.equal(sd["scaling_layer.shift"].flatten(), torch.tensor(H.SHIFT)) and torch.equal(sd["scaling_layer.scale"].flatten(), torch.tensor(H.SCALE))
    lib = _lib.raw()
    for i in (-1, 33, 10_000_000):
        assert lib.dfh_lpips_param_name(ctx, i) == b"" and lib.dfh_lpips_param_ndim(ctx, i) == 0 and lib.dfh_lpips_param_dim(ctx, i, 0) == 0
    assert lib.dfh_lpips_param_dim(ctx, 2, 4) == 0 and lib.dfh_lpips_param_dim(ctx, 2, -1) == 0


def test_packed_and_workspace_sizes_are_the_stated_formulas(ctx):
    lib = _lib.raw()
    assert lib.dfh_lpips_packed_bytes(ctx) == PACKED_BYTES == 58_844_160
    for shape in [(1, 16, 16), (3, 37, 45), (3, 1024, 1024)]:
        assert lib.dfh_lpips_workspace_bytes(ctx, *shape) == workspace_bytes(*shape), shape
    assert lib.dfh_lpips_workspace_bytes(ctx, 1, 15, 16) == 0 and lib.dfh_lpips_workspace_bytes(ctx, 0, 16, 16) == 0
    # the default 4 GiB bound: 3 pairs of outfit sheets, 15 pairs of items
    m = da.LPIPS(init_seed=None)
    assert m.pairs_per_call(1024, 1024) == 3 and m.pairs_per_call(512, 512) == 15
    assert da.LPIPS(init_seed=None, max_workspace_bytes=workspace_bytes(3, 21, 27)).pairs_per_call(21, 27) == 3
    assert da.LPIPS(init_seed=None, max_workspace_bytes=workspace_bytes(3, 21, 27) - 1).pairs_per_call(21, 27) == 2
    with pytest.raises(da.DfhError, match="max_workspace_bytes"):
        da.LPIPS(init_seed=None, max_workspace_bytes=1000).pairs_per_call(16, 16)
    with pytest.raises(ValueError, match="between 16 and 8192"):
        m.pairs_per_call(15, 64)


def test_forward_guards_refuse_on_the_host_before_any_launch(ctx):
    """Made-up addresses, no GPU: count, a null and a misaligned pointer by name, H / W below 16, a small workspace."""
    n, buf = 33, C.c_void_p(8192)
    need = _lib.raw().dfh_lpips_workspace_bytes(ctx, 2, 16, 16)
    good = [4096] * n

    def fwd(params=good, count=n, packed=buf, in0=buf, in1=buf, kind=1, lut=None, norm=0, H_=16, W_=16, dist=buf, ws=buf, ws_bytes=need):
        arr = None if params is None else (C.c_void_p * len(params))(*params)
        return _lib.call("dfh_lpips_forward", ctx, arr, count, packed, in0, in1, kind, lut, norm, 2, H_, W_, dist, None, ws, ws_bytes, None)

    for match, kw in [("count does not match dfh_lpips_num_params", dict(count=n - 1)),
                      ("null argument: params", dict(params=None)),
                      ("null parameter pointer: scaling_layer.scale", dict(params=[4096, 0] + [4096] * (n - 2))),
                      ("not 16-byte aligned: net.slice3.14.bias", dict(params=[4096] * 15 + [4104] + [4096] * (n - 16))),
                      ("not 16-byte aligned: lin4.model.1.weight", dict(params=[4096] * (n - 1) + [4100])),
                      ("null argument: packed", dict(packed=None)), ("null argument: in0", dict(in0=None)), ("null argument: in1", dict(in1=None)),
                      ("null argument: distance", dict(dist=None)), ("null argument: workspace", dict(ws=None)),
                      ("null argument: lut", dict(kind=0)), ("normalize applies to the fp32 form", dict(kind=0, lut=buf, norm=1)),
                      ("src_kind must be", dict(kind=3)),
                      ("packed must be 16-byte aligned", dict(packed=C.c_void_p(8200))), ("in0 must be 16-byte aligned", dict(in0=C.c_void_p(8196))),
                      ("in1 must be 16-byte aligned", dict(in1=C.c_void_p(8204))), ("lut must be 16-byte aligned", dict(kind=0, lut=C.c_void_p(8196))),
                      ("workspace must be 256-byte aligned", dict(ws=C.c_void_p(8192 + 16))),
                      ("at least 16", dict(H_=15)), ("at least 16", dict(W_=8)), ("at most 8192", dict(W_=8200)),
                      ("workspace smaller than dfh_lpips_workspace_bytes", dict(ws_bytes=need - 1))]:
        with pytest.raises(_lib.DfhError, match=match):
            fwd(**kw)
    arr = (C.c_void_p * n)(*good)
    with pytest.raises(_lib.DfhError, match="count does not match"):
        _lib.call("dfh_lpips_pack", ctx, arr, n + 1, buf, None)
    with pytest.raises(_lib.DfhError, match="null argument: packed"):
        _lib.call("dfh_lpips_pack", ctx, arr, n, None, None)
    h = C.c_void_p()
    with pytest.raises(_lib.DfhError, match="only VGG16"):
        _lib.call("dfh_lpips_create", C.byref(_lib.LpipsConfigC(1)), C.byref(h))
    with pytest.raises(_lib.DfhError, match="C_in must be 4"):
        _lib.call("dfh_lpips_conv3x3_relu", buf, buf, 3, buf, buf, buf, 1, 8, 8, 3, 64, None)
    with pytest.raises(_lib.DfhError, match="C_out must be a multiple of 64"):
        _lib.call("dfh_lpips_conv3x3_relu", buf, buf, 4, buf, buf, buf, 1, 8, 8, 4, 32, None)
    with pytest.raises(_lib.DfhError, match=r"C must be in \[1, 512\]"):
        _lib.call("dfh_lpips_layer_score", buf, buf, 1, 4, 4, 1024, buf, buf, None)
    with pytest.raises(_lib.DfhError, match="null argument: scores"):
        _lib.call("dfh_lpips_group_argmin", None, buf, 1, 5, None)


def test_constructor_and_tensor_refusals():
    for kw, match in [(dict(net="alex"), "net='alex'"), (dict(net="squeeze"), "only VGG16"), (dict(version="0.0"), "version="), (dict(lpips=False), "lpips=False"),
                      (dict(spatial=True), "spatial=True"), (dict(pnet_tune=True), "pnet_tune=True"), (dict(eval_mode=False), "eval_mode=False")]:
        with pytest.raises(NotImplementedError, match=match):
            da.LPIPS(init_seed=None, **kw)
    m = da.LPIPS(net="vgg16", pretrained=True, pnet_rand=False, use_dropout=True, verbose=False, init_seed=None)      # the package's keywords; nothing is fetched
    assert m.config == {"net": "vgg", "version": "0.1"} and not m.training and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    assert m.eval() is m
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(x, x)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.lpips_given_data(m, x, x, 2)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.lpips.group_argmin(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="gen holds 2 images, grd 3"):
        da.lpips_given_data(m, x, torch.zeros(3, 3, 16, 16), 2)
    assert np.array_equal(im2tensor_table(), H.im2tensor(torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)).flatten().numpy())


def foreign_state_dicts(params):
    """The two files the package reads, restated from its key layouts: vgg.pth (with the duplicate lins.*) and torchvision's vgg16."""
    lin = {k: v.clone() for k, v in params.items() if k.startswith("lin")}
    lin.update({f"lins.{k}.model.1.weight": params[f"lin{k}.model.1.weight"].clone() for k in range(5)})
    vgg = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v.clone() for k, v in params.items() if k.startswith("net.")}
    vgg.update({"classifier.0.weight": torch.zeros(8, 8), "classifier.0.bias": torch.zeros(8)})
    return lin, vgg


def test_the_three_weight_routes_agree(tmp_path):
    params = H.make_params()
    a = da.LPIPS(init_seed=None)
    a.load_state_dict(params)
    lin, vgg = foreign_state_dicts(params)
    with_dups = dict(params)
    with_dups.update({k: v for k, v in lin.items() if k.startswith("lins.")})
    da.LPIPS(init_seed=None).load_state_dict(with_dups)                          # the package's own state dict carries lins.* too
    b = da.LPIPS(init_seed=None).load_reference_weights(lin, vgg)
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) and torch.equal(b.state_dict()[k], params[k]) for k in params)
    with pytest.raises(KeyError, match="features.28.bias"):
        da.LPIPS(init_seed=None).load_reference_weights(None, {k: v for k, v in vgg.items() if k != "features.28.bias"})
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        da.LPIPS(init_seed=None).load_reference_weights({k: v for k, v in lin.items() if "3" not in k}, None)
    torch.save(lin, str(tmp_path / "vgg.pth"))
    c = da.LPIPS(model_path=str(tmp_path / "vgg.pth"), init_seed=None)
    assert all(torch.equal(c.state_dict()[k], params[k]) for k in params if k.startswith("lin"))
    a.save_pretrained(str(tmp_path / "lpips"))
    assert sorted(os.listdir(tmp_path / "lpips")) == ["config.json", "model.safetensors"]
    d = da.LPIPS.from_pretrained(str(tmp_path), subfolder="lpips", max_workspace_bytes=1 << 30)
    assert d.max_workspace_bytes == 1 << 30 and list(d.state_dict()) == list(params)
    assert all(torch.equal(d.state_dict()[k], params[k]) for k in params)


@pytest.mark.parametrize("name", list(H.CASES))
def test_restatement_reproduces_the_fixtures(name):
    fx = H.load_fixture("lpips_" + name)
    assert os.path.getsize(H.fixture_path("lpips_" + name)) < 16 << 10
    params = H.make_params()
    a, b = H.case_inputs(name)
    np.testing.assert_allclose(fx["checksum"], H.checksum(params, a, b), rtol=1e-12)
    if H.CASES[name][2] == "u8":
        assert a.dtype == torch.uint8 and a.shape == (H.PAIRS, *H.CASES[name][:2], 3)
        a, b = H.im2tensor(a), H.im2tensor(b)
    with torch.no_grad():
        per, total = H.lpips_forward(params, a, b, torch.float32)
    np.testing.assert_allclose(per.numpy(), fx["per_layer32"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(total.numpy(), fx["total32"], rtol=1e-6, atol=0)
    assert fx["per_layer64"].shape == (H.PAIRS, 5) and fx["total64"].shape == (H.PAIRS,) and 1e-3 < float(fx["total64"].min()) < float(fx["total64"].max()) < 1e-1
    # the yardstick the GPU test multiplies by 3 is a real distance, not zero
    assert 0 < H.rel(torch.from_numpy(fx["total32"]), torch.from_numpy(fx["total64"])) < 1e-6


def test_restatement_properties_and_argmin_order():
    params = H.make_params()
    a, b = H.case_inputs("min_16x16")
    with torch.no_grad():
        per, total = H.lpips_forward(params, a[:2], a[:2])
        assert float(total.abs().max()) == 0.0
        pn, tn = H.lpips_forward(params, (a[:2] + 1) / 2, (b[:2] + 1) / 2, torch.float64, normalize=True)
        p0, t0 = H.lpips_forward(params, a[:2], b[:2], torch.float64)
        assert H.rel(tn, t0) < 1e-6
        z = torch.zeros(1, 8, 2, 2)
        assert float(H.layer_score(z, z, torch.ones(1, 8, 1, 1))) == 0.0          # eps outside the root: an all-zero pixel gives 0, not NaN
    rows = torch.from_numpy(H.ARGMIN_ROWS)
    assert np.array_equal(torch.argmin(rows, dim=-1).numpy(), H.argmin_order(H.ARGMIN_ROWS))
    fx = H.load_fixture("lpips_retrieval")
    assert fx["preds"].tolist() == list(H.NEAREST) and abs(float(fx["accuracy"]) - 2 / 3) < 1e-12
    assert np.array_equal(H.argmin_order(fx["scores64"]), fx["preds"])
    gen, cand = H.retrieval_inputs()
    np.testing.assert_allclose(fx["checksum"], H.checksum(params, gen, cand), rtol=1e-12)


def test_table_plan_and_guards_under_the_host_sanitizers(tmp_path):
    """csrc/lpips.hip's host side, built with tests/native/lpips_host_check.hip into a program of its own under
    -fsanitize=address,undefined: the table and the sizes equal the library's, every guard refuses, nothing is launched, no report."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the sanitizer build needs the compiler the library is built with")
    exe = str(tmp_path / "lpips_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(_lib.CSRC, "lpips.hip"),
           os.path.join(ROOT, "tests", "native", "lpips_host_check.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    shapes = [(1, 16, 16), (3, 37, 45), (3, 1024, 1024), (1, 15, 16)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")                      # the HIP runtime's start-up allocations are not ours to free
    r = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    table = [l.split()[2:] for l in lines if l.startswith("param ")]
    assert [(t[0], tuple(map(int, t[1:]))) for t in table] == [(k, tuple(v)) for k, v in H.param_shapes().items()]
    assert f"params 33 floats {sum(int(np.prod(s)) for s in H.param_shapes().values())} packed {PACKED_BYTES}" in lines
    for s in shapes:
        assert f"workspace {s[0]} {s[1]} {s[2]} -> {workspace_bytes(*s) if min(s[1:]) >= 16 else 0}" in lines
    guards = [l for l in lines if l.startswith("guard ")]
    assert len(guards) == 21 and all(": refused (" in l for l in guards), guards
    assert lines[-1] == "launches 0 failures 0"
