"""Writes tests/golden/image_prep.npz: seeded uint8 images and what Pillow's ``Image.resize(..., BILINEAR)`` makes of
them, for tests/test_image_prep_ref.py.  Needs Pillow; the fixture records the version that wrote it.

usage: python tests/helpers/make_image_prep_golden.py"""
import os

import numpy as np

CASES = [((37, 53), (32, 32)), ((20, 24), (32, 64)), ((7, 9), (32, 32)), ((64, 100), (64, 32)), ((50, 70), (45, 33))]


def seeded_image(in_hw, out_hw) -> np.ndarray:
    rng = np.random.default_rng(1000 * in_hw[0] + in_hw[1] + 7 * out_hw[0] + out_hw[1])
    return rng.integers(0, 256, size=in_hw + (3,), dtype=np.uint8)


def pillow_resize(image: np.ndarray, out_hw) -> np.ndarray:
    from PIL import Image

    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(image, "RGB").resize((out_hw[1], out_hw[0]), bilinear))


def main() -> None:
    import PIL

    arrays = {"pillow_version": np.array(PIL.__version__)}
    for i, (in_hw, out_hw) in enumerate(CASES):
        image = seeded_image(in_hw, out_hw)
        arrays["in_%d" % i] = image
        arrays["out_%d" % i] = pillow_resize(image, out_hw)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "image_prep.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
