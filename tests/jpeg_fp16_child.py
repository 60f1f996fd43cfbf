"""Child-process body of tests/test_gpu_jpeg.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a property of the
process (tests/fp16_child.py), so the round trip of a few cases runs here under DFH_STORAGE=fp16 (``python -m tests.jpeg_fp16_child``)
and prints the digests of its results as one line ``JPEG_FP16_RESULT {...}``."""
import json

import numpy as np
import torch

import difashion_amd as da
from tests import helpers_jpeg as H
from tests.gpu_util import DEV

CASES = [(17, 23, 75, "4:2:0"), (30, 46, 1, "4:2:0"), (100, 75, 100, "4:4:4")]


def case(device):
    """The shared cases of parent and child -> the sha256 of pixels and coefficients per case, uint8 and fp32 source."""
    out = {}
    for h, w, quality, subsampling in CASES:
        images = np.stack([H.case_image(kind, h, w) for kind in H.KINDS])
        px, coef = da.jpeg_roundtrip(torch.from_numpy(images).to(device), quality, subsampling, return_coefficients=True)
        x = torch.from_numpy(images).to(device).permute(0, 3, 1, 2).float() / 127.5 - 1.0
        fpx = da.jpeg_roundtrip(x.contiguous(), quality, subsampling)
        key = f"{h}x{w}_{H.setting_id((quality, subsampling))}"
        out[key] = [H.checksum(px.cpu().numpy()), H.checksum(coef.cpu().numpy()), H.checksum(fpx.cpu().numpy())]
    return out


def main():
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    print("JPEG_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(),
                                            "digests": case(DEV)}), flush=True)


if __name__ == "__main__":
    main()
