"""-m gpu: the item store on the device.  dfh_item_gather and dfh_history_rows bit for bit against the torch
expressions they replace and the checked sequential emulation (tests/helpers_item_store.py), within the derived bound of fp64, past
2^31 elements, in both storage libraries; the store against the real tiny AutoencoderKL; DiFashion.forward and fashion_generation
through store + table against the image + dict path, bit for bit under the same seeds."""
import functools
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import difashion_amd as da
from difashion_amd.difashion import DiFashion
from tests import helpers_item_store as H
from tests.gpu_util import DEV, release_cached_gpu_memory
from tests.helpers import GLUE_CFG, glue_unet_params, load
from tests.helpers_data import synthetic_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
d = lambda t: t.to(DEV)


@functools.lru_cache(maxsize=None)
def tables(row_elems):
    """Per row size: the random and the exact-data table on the host and the device, the segments, the null row.  Shared, never written."""
    table, exact = H.make_table(H.ITEMS, row_elems, seed=3), H.make_table(H.ITEMS, row_elems, seed=4, exact=True)
    segs = H.make_segments(H.ITEMS, seed=5)
    null = torch.full((row_elems,), 0.25)
    assert H.exact_condition(exact, row_elems, segs, 1.0)
    return table, exact, d(table), d(exact), segs, null


@pytest.mark.parametrize("rows", H.ROWS)
@pytest.mark.parametrize("row_elems", H.ROW_ELEMS)
def test_item_gather_is_the_torch_expression_bit_for_bit(row_elems, rows):
    table, _, table_d, _, _, _ = tables(row_elems)
    ids = H.gather_ids(rows, H.ITEMS, seed=6 + rows)
    eps = torch.randn(rows, row_elems, generator=torch.Generator().manual_seed(7))
    mean, std = table[:, :row_elems], table[:, row_elems:]
    got = H.run_gather(table_d, row_elems, d(ids), d(eps), H.SCALE)
    assert H.same_bits(got, (mean[ids] + std[ids] * eps) * H.SCALE)                 # latent_dist.sample() * sf
    mode = H.run_gather(table_d, row_elems, d(ids), None, H.SCALE)
    assert H.same_bits(mode, mean[ids] * H.SCALE)                                   # latent_dist.mode() * sf
    # a means-only table (row_stride == row_elems) is legal without eps
    means_only = d(mean.contiguous())
    assert H.same_bits(H.run_gather(means_only, row_elems, d(ids), None, 1.0), mean[ids])
    with pytest.raises(da.DfhError, match=r"row_stride smaller than 2 \* row_elems"):
        H.run_gather(means_only, row_elems, d(ids), d(eps), 1.0)
    # a rerun, and the rows split over two calls, give the same bits
    assert H.same_bits(H.run_gather(table_d, row_elems, d(ids), d(eps), H.SCALE), got)
    if rows > 1:
        cut = rows // 2
        parts = [H.run_gather(table_d, row_elems, d(ids[a:b]), d(eps[a:b].contiguous()), H.SCALE) for a, b in ((0, cut), (cut, rows))]
        assert H.same_bits(torch.cat(parts), got)


@pytest.mark.parametrize("row_elems", H.ROW_ELEMS)
def test_item_gather_out_of_range_id_is_a_nan_row(row_elems):
    table, _, table_d, _, _, _ = tables(row_elems)
    ids = torch.tensor([3, H.ITEMS, 0, -1, H.ITEMS - 1, 2 ** 40])
    eps = torch.randn(len(ids), row_elems, generator=torch.Generator().manual_seed(8))
    for e in (eps, None):
        out = torch.full((len(ids) + 2, row_elems), 7.0, device=DEV)                # a guard row either side
        H.run_gather(table_d, row_elems, d(ids), None if e is None else d(e), H.SCALE, out=out[1:-1])
        want = H.emulate_gather(table, row_elems, ids.clamp(-1, H.ITEMS), e, H.SCALE)
        got = out.cpu()
        assert bool((got[0] == 7.0).all()) and bool((got[-1] == 7.0).all())
        for r in range(len(ids)):
            if 0 <= int(ids[r]) < H.ITEMS:
                assert H.same_bits(got[1 + r], want[r]), r                          # the neighbours are untouched
            else:
                assert bool(got[1 + r].isnan().all()), r


@pytest.mark.parametrize("rows", H.ROWS)
@pytest.mark.parametrize("row_elems", H.ROW_ELEMS)
def test_history_rows_sequential_exact_and_fp64(row_elems, rows):
    table, exact, table_d, exact_d, segs, null = tables(row_elems)
    row_seg = H.row_segments(rows)
    dev = H.history_device_inputs(segs, row_seg, DEV)
    got = H.run_history(table_d, row_elems, *dev, d(null), H.SCALE)
    # 2. bit-equal to the sequential emulation on random data ...
    assert H.same_bits(got, H.emulate_history(table, row_elems, segs, row_seg, null, H.SCALE))
    # ... and to torch.mean of the gathered rows on exact data (integer latents, scale 1: every partial sum is exact)
    got_exact = H.run_history(exact_d, row_elems, *dev, d(null), 1.0)
    assert H.same_bits(got_exact, H.torch_mean_history(exact, row_elems, segs, row_seg, null))
    # 3. every element within (L + 1) 2^-24 mean_k |scale x_k| of fp64
    ref, bound = H.history_ref64(table, row_elems, segs, row_seg, null, H.SCALE)
    err = (got.cpu().double() - ref).abs()
    live = bound > 0
    if bool(live.any()):
        print(f"history rows {rows} x {row_elems}: worst error / bound {float((err[live] / bound[live]).max()):.3f}")
    assert bool((err <= bound).all())
    # 8. a rerun, and the rows split over two calls, give the same bits
    assert H.same_bits(H.run_history(table_d, row_elems, *dev, d(null), H.SCALE), got)
    if rows > 1:
        cut = rows // 2
        parts = [H.run_history(table_d, row_elems, dev[0], dev[1], dev[2][a:b].contiguous(), d(null), H.SCALE) for a, b in ((0, cut), (cut, rows))]
        assert H.same_bits(torch.cat(parts), got)


def test_history_rows_null_alone_and_means_only_table():
    row_elems = 256
    table, _, table_d, _, segs, null = tables(row_elems)
    seg_items, seg_offsets, _ = H.history_device_inputs(segs, [0], DEV)
    alone = H.run_history(table_d, row_elems, seg_items, seg_offsets, torch.tensor([-1], dtype=torch.int32, device=DEV), d(null), H.SCALE)
    assert H.same_bits(alone, null[None])
    empty = H.run_history(table_d, row_elems, seg_items, seg_offsets, torch.tensor([6], dtype=torch.int32, device=DEV), d(null), H.SCALE)
    assert H.same_bits(empty, null[None])
    means_only = d(table[:, :row_elems].contiguous())                               # only the first row_elems floats of a row are read
    row_seg = H.row_segments(5)
    got = H.run_history(means_only, row_elems, *H.history_device_inputs(segs, row_seg, DEV), d(null), H.SCALE)
    assert H.same_bits(got, H.emulate_history(table, row_elems, segs, row_seg, null, H.SCALE))


def test_rows_past_two_to_the_31_elements():
    """65 540 rows x 32 768 floats: the last rows start beyond 2^31 elements (and 2^33 bytes).  Only they are written."""
    items, stride, row_elems = 65540, 32768, 16384
    release_cached_gpu_memory()
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("less than 12 GB of device memory free")
    assert (items - 3) * stride > 2 ** 31
    small = H.make_table(3, row_elems, seed=12)
    big = torch.empty((items, stride), dtype=torch.float32, device=DEV)
    big[items - 3:] = d(small)
    ids = torch.tensor([items - 3, items - 1, items - 2, items - 1])
    eps = torch.randn(len(ids), row_elems, generator=torch.Generator().manual_seed(13))
    assert H.same_bits(H.run_gather(big, row_elems, d(ids), d(eps), H.SCALE), H.emulate_gather(small, row_elems, ids - (items - 3), eps, H.SCALE))
    assert H.same_bits(H.run_gather(big, row_elems, d(ids), None, H.SCALE), H.emulate_gather(small, row_elems, ids - (items - 3), None, H.SCALE))
    past = H.run_gather(big, row_elems, d(torch.tensor([items - 1, items])), None, H.SCALE).cpu()
    assert H.same_bits(past[0], small[2, :row_elems] * H.SCALE) and bool(past[1].isnan().all())
    segs, row_seg, null = [[items - 3, items - 2, items - 1, items - 3, items - 1]], [0, -1], torch.full((row_elems,), 0.25)
    got = H.run_history(big, row_elems, *H.history_device_inputs(segs, row_seg, DEV), d(null), H.SCALE)
    assert H.same_bits(got, H.emulate_history(small, row_elems, [[0, 1, 2, 0, 2]], row_seg, null, H.SCALE))
    del big
    release_cached_gpu_memory()


def test_store_and_table_api_on_the_preprocessing_cache():
    """from_latents on the device: a means-only store with scale 1; the HistoryTable of the synthetic data set through the Python API."""
    _, _, history, latents = synthetic_dataset()
    store = da.ItemLatentStore.from_latents(latents, 0.18215, device=DEV)
    ids = torch.tensor([12, 0, 5, 5])
    assert H.same_bits(store.modes(ids), latents[ids]) and H.same_bits(store.modes(d(ids)), latents[ids])
    assert H.same_bits(store.null_latent(), latents[0])
    bad = store.modes(d(torch.tensor([1, 13]))).cpu()                               # ids on the device are not synced for a check
    assert H.same_bits(bad[0], latents[1]) and bool(bad[1].isnan().all())
    ht = da.HistoryTable(history, store)
    uids, cates = [7, 9, 8, 7, 9], [torch.tensor(5), 3, 1, 3, torch.tensor(4)]
    segs = [history[7][1], history[7][2], history[7][5], history[9][3], history[9][4]]
    assert ht.segment_ids(uids, cates) == [2, 3, -1, -1, 4]
    flat = latents.reshape(13, -1)
    got = ht.rows(uids, cates, store.null_latent())
    assert got.shape == (5, 4, 8, 8)
    assert H.same_bits(got.reshape(5, -1), H.emulate_history(flat, 256, segs, [2, 3, -1, -1, 4], flat[0], 1.0))
    off = ht.rows(uids, cates, store.null_latent(), use_history=False)
    assert H.same_bits(off, latents[0][None].expand(5, -1, -1, -1).contiguous())


def test_store_equals_the_real_tiny_vae_on_its_build_batches():
    vae = da.AutoencoderKL(block_out_channels=(32, 64, 64, 64), sample_size=32).to(DEV)
    sf = vae.config.scaling_factor
    imgs = torch.rand(12, 3, 32, 32, generator=torch.Generator().manual_seed(21)) * 2 - 1
    store = da.ItemLatentStore.build(vae, imgs, DEV, batch_size=4)
    assert len(store) == 12 and store.latent_shape == (4, 4, 4) and store.has_std and store.scale == sf and store.nbytes == 12 * 128 * 4
    assert da.data.build_item_store(vae, imgs, DEV, batch_size=4).table.equal(store.table)
    for k in range(3):
        ids = list(range(4 * k, 4 * k + 4))
        dist = vae.encode(d(imgs[ids])).latent_dist
        assert H.same_bits(store.modes(ids), dist.mode() * sf)
        torch.manual_seed(50 + k)
        want = vae.encode(d(imgs[ids])).latent_dist.sample() * sf
        after_want = torch.rand(1, device=DEV)
        torch.manual_seed(50 + k)
        got = store.sample(ids)
        assert H.same_bits(got, want)
        assert torch.equal(torch.rand(1, device=DEV), after_want)                   # the RNG stream was consumed identically
        g1, g2 = torch.Generator(device=DEV).manual_seed(9), torch.Generator(device=DEV).manual_seed(9)
        assert H.same_bits(store.sample(torch.tensor(ids), generator=g1), dist.sample(g2) * sf)


# ---------------------------------------------------------------------- DiFashion through the store
from tests.test_gpu_difashion import CATE_NUM, TableText, TensorKeyDict, ZeroTok  # noqa: E402
from tests.test_gpu_pipeline import encoder  # noqa: E402
from tests.test_gpu_unet import hip_unet  # noqa: E402

HS = GLUE_CFG.sample_size
N_ITEMS = 40


@pytest.fixture(scope="module")
def glue():
    """The GLUE-size model with a stand-in VAE that has a real posterior, the item table, its store, and the history in both forms:
    the HistoryTable and a TensorKeyDict holding the table's own per-segment rows."""
    unet = hip_unet(GLUE_CFG, glue_unet_params(), max_batch=32)
    rec = load("train_b2_mse.npz")
    vae = H.PosteriorVAE(HS, DEV)
    g = torch.Generator().manual_seed(41)
    dataset = torch.randn(N_ITEMS, 4, HS, HS, generator=g) * 0.6
    store = da.ItemLatentStore.build(vae, dataset, DEV, batch_size=16)
    uids = torch.arange(8) + 100
    raw = {int(u): {c: torch.randint(0, N_ITEMS, (1 + (int(u) + c) % 6,), generator=g).tolist() for c in range(1, CATE_NUM, 2)} for u in uids}
    table = da.HistoryTable(raw, store)
    null = store.null_latent()
    as_dict = {u: TensorKeyDict({c: table.rows([u], [c], null)[0] for c in per}) for u, per in raw.items()}
    return types.SimpleNamespace(unet=unet, rec=rec, vae=vae, dataset=dataset, store=store, uids=uids, table=table, as_dict=as_dict)


def model(glue, sched):
    args = types.SimpleNamespace(use_history=True, use_mutual_guidance=True, eta=0.1, snr_gamma=5.0, noise_offset=0)
    return DiFashion(args, vae=glue.vae, unet=glue.unet, fashion_encoder=encoder(glue.rec), noise_scheduler=sched, text_encoder=TableText(),
                     tokenizer=ZeroTok())


@pytest.mark.parametrize("bsz", [2, 8])
def test_forward_through_store_and_table_is_bit_identical(glue, bsz):
    g = torch.Generator().manual_seed(60 + bsz)
    outfits = torch.randint(0, N_ITEMS, (bsz, 4), generator=g)
    cats = torch.randint(1, CATE_NUM, (bsz, 4), generator=g)                        # odd categories have history, even ones fall to null
    ids = torch.zeros(bsz, 4, 77, dtype=torch.long)
    ids[:, :, 0] = cats + 5
    batch = dict(uids=glue.uids[:bsz], outfits=outfits, category=cats, input_ids=ids)
    m = model(glue, da.DDIMScheduler())

    def run(img_dataset, history, null_img):
        taps = {}
        torch.manual_seed(1234 + bsz)
        with torch.no_grad():
            loss = m(batch, img_dataset, history, null_img, 0.2, 0.3, 0.2, torch.float32, torch.Generator(device=DEV).manual_seed(77), taps=taps)
        return taps["x_in"].clone(), taps["timesteps"].clone(), loss.detach().clone()

    base = run(glue.dataset, glue.as_dict, glue.dataset[0])                         # the image + dict path
    assert bool(torch.isfinite(base[2])) and bool(base[0][:, 4:].abs().sum() > 0)
    for name, got in (("store + table", run(glue.store, glue.table, None)), ("store + dict", run(glue.store, glue.as_dict, None)),
                      ("images + table", run(glue.dataset, glue.table, glue.dataset[0])),
                      ("store + table, null image encoded", run(glue.store, glue.table, glue.dataset[0]))):
        assert H.same_bits(got[0], base[0]), name
        assert torch.equal(got[1], base[1]), name
        assert H.same_bits(got[2].reshape(1), base[2].reshape(1)), name


@pytest.mark.parametrize("ol", [[[3, 0, 5, 6], [7, 8, 9, 0]], [[0, 0, 0, 0]]], ids=["fitb", "gor"])
def test_fashion_generation_from_the_store_is_bit_identical(glue, ol):
    olists = torch.tensor(ol)
    bsz = len(ol)
    g = torch.Generator().manual_seed(70 + bsz)
    cats = torch.randint(1, CATE_NUM, (bsz, 4), generator=g)
    ids = torch.zeros(bsz, 4, 77, dtype=torch.long)
    ids[:, :, 0] = cats + 5
    uids, oids = glue.uids[:bsz], torch.arange(bsz) + 900
    init = torch.randn(int((olists == 0).sum()), 4, HS, HS, generator=g)
    m = model(glue, da.DDIMScheduler())
    common = dict(uids=uids, oids=oids, input_ids=ids, olists=olists, category=cats, num_inference_steps=6, category_guidance_scale=12.0,
                  hist_guidance_scale=4.0, mutual_guidance_scale=5.0, eta=0.0, init_latents=d(init), output_type="latent", return_dict=True)
    base = m.fashion_generation(outfit_images=d(glue.dataset[olists.reshape(-1)]), history=glue.as_dict, null_img=d(glue.dataset[0]), **common)
    got = m.fashion_generation(outfit_images=None, item_store=glue.store, history=glue.table, null_img=None, **common)
    assert bool(torch.isfinite(base[0].images).all())
    assert H.same_bits(got[0].images, base[0].images)
    for a, b in zip(got[1:], base[1:]):
        assert torch.equal(a, b)


def test_fp16_storage_library_gives_the_same_bits():
    """The kernels are fp32 only: libdifashion_hip_f16.so, in a process of its own, gives the bits of the bf16 build."""
    from tests.item_store_fp16_child import case
    gathered, hist = case(DEV)
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.item_store_fp16_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ITEM_STORE_FP16_RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("ITEM_STORE_FP16_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"]
    assert res["gather"] == H.bits(gathered).flatten().tolist() and res["history"] == H.bits(hist).flatten().tolist()
