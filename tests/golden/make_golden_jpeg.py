"""Writes tests/golden/jpeg_roundtrip.npz: what the REAL PIL gives for the JPEG save / open round trip of the
seeded case images of tests/helpers_jpeg.py, for the sizes up to 100 x 75.  Per case the round-tripped uint8 image and the sha256 of the
input it was made from (the tests regenerate the inputs from the seeds).  tests/test_jpeg_cpu.py holds the numpy restatement to this
file, so the arithmetic contract survives an upgrade of PIL / libjpeg.

    python -m tests.golden.make_golden_jpeg
"""
import numpy as np
import PIL
from PIL import features

from tests import helpers_jpeg as H


def main():
    assert features.check_feature("libjpeg_turbo"), "the fixture is made with libjpeg-turbo, the library PIL's wheels ship"
    out = {"pil_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(str(features.version_feature("libjpeg_turbo")))}
    for case in H.golden_cases():
        kind, h, w, quality, subsampling = case
        a = H.case_image(kind, h, w)
        key = H.golden_key(*case)
        out[key] = H.pil_roundtrip(a, quality, subsampling)
        out[key + "_input_sha256"] = np.array(H.checksum(a))
    np.savez_compressed(H.GOLDEN, **out)
    print(f"wrote {H.GOLDEN}: {len(out)} arrays")


if __name__ == "__main__":
    main()
