"""Not a test: a small `--dataset frames` tree written with Pillow at test time, shared by tests/test_resample_host.py and
tests/test_gpu_frames.py.

    <root>/train/a/frame<k>.png          6 frames 30 x 40 (H x W), RGB, named frame0 .. frame5 (frame10 sorts after frame2: see `b`)
    <root>/train/b/deep/f<k>.png         12 frames 30 x 40 RGB named f0 .. f11: nested, natural order
    <root>/train/c/<k>.jpg               7 frames 48 x 48, a grey picture saved as an RGB JPEG
    <root>/train/short/<k>.png           2 frames: too short for any clip the tests draw
    <root>/train/empty/                  no frame: ignored
    <root>/test/x/<k>.png, test/y/<k>.png   5 frames 30 x 40 RGB each
"""
import os

import numpy as np
from PIL import Image

CLIPS = {
    "train": [("a", "frame%d.png", 6, (30, 40)), (os.path.join("b", "deep"), "f%d.png", 12, (30, 40)), ("c", "%d.jpg", 7, (48, 48)),
              ("short", "%d.png", 2, (30, 40))],
    "test": [("x", "%d.png", 5, (30, 40)), ("y", "%d.png", 5, (30, 40))],
}


def frame(seed, split, clip, k, hw, grey=False):
    """(H, W, 3) uint8: a smooth moving pattern plus noise, so that every filter has something to do."""
    h, w = hw
    rng = np.random.default_rng([seed, split == "test", sum(map(ord, clip)), k])
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 100.0 * np.sin((xx + 3 * k) / 5.0) * np.cos((yy - 2 * k) / 4.0)
    img = base[..., None] + rng.normal(0, 25, (h, w, 1 if grey else 3))
    return np.clip(np.broadcast_to(img, (h, w, 3)), 0, 255).astype(np.uint8)


def build(root, seed=5):
    """Writes the tree under `root` (a --data_root) and returns str(root)."""
    root = str(root)
    for split, clips in CLIPS.items():
        for clip, pattern, n, hw in clips:
            d = os.path.join(root, split, clip)
            os.makedirs(d, exist_ok=True)
            for k in range(n):
                im = Image.fromarray(frame(seed, split, clip, k, hw, grey=pattern.endswith(".jpg")))
                im.save(os.path.join(d, pattern % k), **({"quality": 90} if pattern.endswith(".jpg") else {}))
    os.makedirs(os.path.join(root, "train", "empty"), exist_ok=True)
    return root


def pillow_pool(index, size, filter, fit):
    """(n_frames, S, S, C) uint8: every file of the index through Pillow's own resize - the oracle of both pool builders."""
    from dvg_amd import resample
    out = []
    for f in (f for seq in index.sequences for f in seq):
        with Image.open(f) as im:
            if im.size != (size, size):
                im = im.resize((size, size), resample.pil_filter(filter), box=resample.fit_box(im.size[0], im.size[1], size, size, fit))
            out.append(np.asarray(im).reshape(size, size, -1))
    return np.stack(out)
