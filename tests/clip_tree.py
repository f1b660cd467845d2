"""A tiny deterministic dataset tree in the three on-disk formats the reference's loaders read (data/kth.py, data/ucf.py,
data/bair.py), written with Pillow at test time.  Not a test: tests/test_clip_datasets.py, tests/test_gpu_clips.py and
tests/golden/make_golden_clips.py build it.

    <root>/kth/processed/<class>/{train,test}_meta64x64.json + <class>/<vid>/image-NNN_64x64.png   six classes, RGB PNGs with
                                                                 three equal channels (as the KTH converter writes them)
    <root>/ucf/processed/<class>/{train,test}_meta64x64.pt   + <class>/<vid>/image-NNN_64x64.png   nine classes, true RGB
    <root>/bair/processed_data/{train,test}/<d1>/<d2>/<i>.png                                      2 x 3 directories, RGB

Every frame is seeded noise keyed by (dataset, class, video, sequence, frame): no two frames are equal, so a clip's CRC names
its sequence and start.  Some KTH / UCF sequences are shorter than the T = 8 of the fixture (the re-draw loop)."""
import json
import os

import numpy as np
import torch

SIZE = 64
KTH_CLASSES = ['boxing', 'handclapping', 'handwaving', 'jogging', 'running', 'walking']
UCF_CLASSES = ['BenchPress', 'BodyWeightSquats', 'CleanAndJerk', 'PullUps', 'PushUps', 'Shotput', 'TennisSwing', 'Lunges',
               'Fencing']
LENGTHS = (5, 9, 12, 14, 16, 6, 13)      # cycled over the sequences: 5 and 6 are shorter than T = 8
BAIR_FRAMES = 12
DATASETS = ('kth', 'ucf', 'bair')


def frame(seed, dataset, c, v, s, f, rgb):
    """(64,64,3) uint8; rgb False: one channel of noise in all three."""
    rng = np.random.default_rng([seed, DATASETS.index(dataset), c, v, s, f])
    if rgb:
        return rng.integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)
    return np.repeat(rng.integers(0, 256, (SIZE, SIZE, 1), dtype=np.uint8), 3, axis=2)


def _save(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path, compress_level=1)


def _meta_tree(root, seed, dataset, classes, n_videos, rgb, dump):
    k = 0
    for c, cname in enumerate(classes):
        cdir = os.path.join(root, dataset, 'processed', cname)
        v = 0
        for split in ('train', 'test'):
            meta = []
            for _ in range(n_videos[split]):
                vid = 'person%02d_%s_d%d' % (v + 1, cname, 1 + v % 4)
                os.makedirs(os.path.join(cdir, vid), exist_ok=True)
                files, n = [], 0
                for s in range(2):
                    names = []
                    for f in range(LENGTHS[k % len(LENGTHS)]):
                        names.append('image-%03d_%dx%d.png' % (n, SIZE, SIZE))
                        _save(os.path.join(cdir, vid, names[-1]), frame(seed, dataset, c, v, s, f, rgb))
                        n += 1
                    files.append(names)
                    k += 1
                meta.append({'vid': vid, 'files': files})
                v += 1
            dump(meta, os.path.join(cdir, '%s_meta%dx%d' % (split, SIZE, SIZE)))


def _dump_json(meta, path):
    with open(path + '.json', 'w') as f:
        json.dump(meta, f)


def build(root, seed=0):
    """Writes the three trees under root/kth, root/ucf, root/bair (each a --data_root) and returns root."""
    root = str(root)
    _meta_tree(root, seed, 'kth', KTH_CLASSES, {'train': 3, 'test': 2}, False, _dump_json)
    _meta_tree(root, seed, 'ucf', UCF_CLASSES, {'train': 2, 'test': 1}, True, lambda m, p: torch.save(m, p + '.pt'))
    for c, split in enumerate(('train', 'test')):
        for v, d1 in enumerate(('traj_0_to_255', 'traj_256_to_511')):
            for s in range(3):
                d = os.path.join(root, 'bair', 'processed_data', split, d1, str(s + 3 * v))
                os.makedirs(d)
                for f in range(BAIR_FRAMES):
                    _save(os.path.join(d, '%d.png' % f), frame(seed, 'bair', c, v, s, f, True))
    return root


def data_root(root, dataset):
    return os.path.join(str(root), dataset)
