"""Write tests/golden/augment_post_pil.json: what PIL itself gives for the post stage of the clip transforms (bvc_frame_post), so that
the suite can hold the library to Pillow's bytes where PIL is not installed.

    python tools/make_augment_post_golden.py

Two 16 x 24 x 3 uint8 frames (tests/augment_post_ref.frames, seed 7) and, for both of them, ImageFilter.GaussianBlur at radii 0.3, 1.0,
2.0 and 4.0 and Image.rotate(NEAREST, expand=False, fillcolor=0) by -90, -37.5, 1e-3, 45 and 90 degrees; for the first frame also
GaussianBlur(1.3) followed by rotate(30).  Arrays are [3, H, W] uint8, base64 of their bytes.  The PIL version is recorded.
"""
import base64
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augment_post_ref as P   # noqa: E402

H, W = 16, 24
RADII = [0.3, 1.0, 2.0, 4.0]
ANGLES = [-90.0, -37.5, 1e-3, 45.0, 90.0]


def b64(a):
    return base64.b64encode(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).decode()


def main():
    import PIL
    x = P.frames(2, H, W, seed=7).numpy()
    cases = []
    for i in range(2):
        for r in RADII:
            cases.append({"frame": i, "radius": r, "angle": None, "out": b64(P.pil_blur(x[i], r))})
        for a in ANGLES:
            cases.append({"frame": i, "radius": None, "angle": a, "out": b64(P.pil_rotate(x[i], a))})
    cases.append({"frame": 0, "radius": 1.3, "angle": 30.0, "out": b64(P.pil_rotate(P.pil_blur(x[0], 1.3), 30.0))})
    doc = {"pil_version": PIL.__version__, "shape": [3, H, W], "frames": [b64(x[0]), b64(x[1])], "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "augment_post_pil.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0)
        fh.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(cases)} cases, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
