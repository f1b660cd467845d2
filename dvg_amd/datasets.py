"""KTH, BAIR and UCF clips from `--data_root`: the on-disk formats of the reference's loaders (data/kth.py, data/bair.py,
data/ucf.py) indexed on the host, every indexed PNG decoded ONCE into a device-resident uint8 frame pool, and samplers that
reproduce the reference's random draws.  A batch is then B pool indices: `ops.clip_gather` (dvg_clip_gather_u8) turns them
into normalize_data's list of T x (B,C,H,W) float32 frames on the device.  Host code, no GPU at import.

    KTH   <root>/processed/<class>/{train,test}_meta<S>x<S>.json   a list of {'vid', 'files': [[names...], ...]}; the frames
          are <root>/processed/<class>/<vid>/<name> (kth.py:16-17,30-32,47-53)
    UCF   the same tree with .pt metas read by torch.load and nine classes (ucf.py:17,31); ucf.py:13 sets `train = True`
          whatever it is given, so the UCF test split IS the train split - kept
    BAIR  <root>/processed_data/{train,test}/<d1>/<d2>/<i>.png, i = 0, 1, ... (bair.py:17-26,53)

    frames  <root>/{train,test}/.../<clip>/<frame>.{png,jpg,jpeg}: every directory below a split that directly holds at least one
          such file is one clip (nested freely); clips sorted by path, frames in natural order (frame2 before frame10).  Not a
          format of the reference: a folder of clips as a camera or a frame dump leaves it, frames of ANY size - see `--resize`

`--resize FILTER` (docs/DESIGN_NOTES_frames.md): a decoded frame that is not image_width x image_width is scaled as Pillow's
`Image.resize` scales it - on the device while the pool is built (`ops.resample_u8`, dvg_resample_u8: bit-equal to Pillow), by
Pillow itself for a host pool.  It applies to every dataset read here; without it a frame of another size is refused, as ever.

Deviation: the reference lists the BAIR directories with os.listdir, whose order depends on the file system; here they are
listed SORTED, so the ordered test walk and the train draws name the same directories on every machine.

Out of scope: the download scripts and the Lua / ffmpeg / TFRecord converters that make the reference's trees (what they do
for the model - scaling the frames - is `--resize`), video containers, a cache of the decoded pool on disk, and datasets
larger than the device memory (the pool holds every indexed frame: BAIR at 64x64 is about 16 GB)."""
from __future__ import annotations

import argparse
import json
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import resample

KTH_CLASSES = ['boxing', 'handclapping', 'handwaving', 'jogging', 'running', 'walking']                      # kth.py:16-17
UCF_CLASSES = ['BenchPress', 'BodyWeightSquats', 'CleanAndJerk', 'PullUps', 'PushUps', 'Shotput', 'TennisSwing', 'Lunges',
               'Fencing']                                                                                    # ucf.py:17-18
REAL_DATASETS = ('kth', 'bair', 'ucf', 'frames')
FRAME_EXTENSIONS = ('.png', '.jpg', '.jpeg')
STAGING_BYTES = 256 << 20       # the pinned staging buffer of build_pool, at most
MAX_DECODE_THREADS = 16


def _need(path, what):
    """A missing piece of the tree ends the program with its path, not with a traceback."""
    if not os.path.exists(path):
        raise SystemExit(f"dataset: {what} {path!r} does not exist (--data_root must hold the reference's processed tree)")
    return path


class ClipIndex:
    """The sequences of one split: `sequences[i]` = the frame files of sequence i in order, `labels[i]` its class label
    (-1: BAIR has none).  `bases[i]` = the pool index of its first frame once the frames are laid out sequence after
    sequence (build_pool does).  KTH / UCF also keep `videos[c]` = per class, per video, the sequence ids: the nesting the
    reference draws from."""

    def __init__(self, dataset, split):
        self.dataset, self.split = dataset, split
        self.sequences, self.labels, self.videos = [], [], []

    def _add(self, files, label):
        self.sequences.append(files)
        self.labels.append(label)
        return len(self.sequences) - 1

    @property
    def lengths(self):
        return np.array([len(s) for s in self.sequences], np.int64)

    @property
    def bases(self):
        n = self.lengths
        return np.cumsum(n) - n

    @property
    def n_frames(self):
        return int(self.lengths.sum())


def _meta_index(dataset, root, train, image_width, classes, load, ext):
    base = _need(os.path.join(_need(root, "--data_root"), "processed"), "directory")
    split = 'train' if train else 'test'
    idx = ClipIndex(dataset, split)
    for label, c in enumerate(classes):
        cdir = _need(os.path.join(base, c), "class directory")
        meta = load(_need(os.path.join(cdir, '%s_meta%dx%d.%s' % (split, image_width, image_width, ext)), "meta file"))
        vids = []
        for vid in meta:
            vdir = os.path.join(cdir, vid['vid'])
            vids.append([idx._add([os.path.join(vdir, f) for f in files], label) for files in vid['files']])
        if not vids:
            raise SystemExit(f"dataset: class {c!r} of the {dataset} {split} split under {base!r} lists no video")
        idx.videos.append(vids)
    return idx


def kth_index(root, train, image_width=64):
    def load(path):
        with open(path) as f:
            return json.load(f)
    return _meta_index('kth', root, train, image_width, KTH_CLASSES, load, 'json')


def ucf_index(root, train, image_width=64):
    # ucf.py:13 `train = True`: both splits read the train metas
    return _meta_index('ucf', root, True, image_width, UCF_CLASSES, lambda p: torch.load(p, weights_only=True), 'pt')


def bair_index(root, train, image_width=64):
    split = 'train' if train else 'test'
    base = _need(os.path.join(_need(root, "--data_root"), "processed_data", split), "directory")
    idx = ClipIndex('bair', split)
    for d1 in sorted(os.listdir(base)):
        for d2 in sorted(os.listdir(os.path.join(base, d1))):
            d = os.path.join(base, d1, d2)
            n = 0
            while os.path.exists(os.path.join(d, '%d.png' % n)):
                n += 1
            idx._add([os.path.join(d, '%d.png' % i) for i in range(n)], -1)
    if not idx.sequences:
        raise SystemExit(f"dataset: no <d1>/<d2> directory under {base!r}")
    return idx


def _natural(name):
    """The sort key of a natural order: digit runs compare as numbers (frame2 before frame10)."""
    return [(0, int(t), '') if t.isdigit() else (1, 0, t) for t in re.split(r'(\d+)', name) if t]


def frames_index(root, train, image_width=64):
    """A folder of clips: every directory below <root>/train (or /test) that directly holds at least one .png / .jpg / .jpeg file
    is one clip, its frames in natural order; clips sorted by path.  Frames may have any size (`--resize`); no labels."""
    split = 'train' if train else 'test'
    base = _need(os.path.join(_need(root, "--data_root"), split), "directory")
    idx = ClipIndex('frames', split)
    for d, subdirs, names in os.walk(base):
        subdirs.sort()                                      # clips sorted by path, on every file system
        frames = sorted((f for f in names if f.lower().endswith(FRAME_EXTENSIONS)), key=lambda f: (_natural(f), f))
        if frames:
            idx._add([os.path.join(d, f) for f in frames], -1)
    if not idx.sequences:
        raise SystemExit(f"dataset: no directory with .png / .jpg / .jpeg frames under {base!r}")
    order = sorted(range(len(idx.sequences)), key=lambda i: os.path.dirname(idx.sequences[i][0]))
    idx.sequences = [idx.sequences[i] for i in order]
    return idx


def open_index(dataset, root, train, image_width=64):
    if dataset not in REAL_DATASETS:
        raise SystemExit(f"dataset: no loader for {dataset!r} (kth | bair | ucf | frames)")
    return {'kth': kth_index, 'ucf': ucf_index, 'bair': bair_index, 'frames': frames_index}[dataset](root, train, image_width)


class MetaSampler:
    """KTH / UCF: get_sequence's draws in its order (kth.py:37-48, ucf.py:38-52).  Class, video and sequence come from a
    np.random.RandomState(seed), drawn again while the sequence is shorter than the clip; the start frame from
    random.Random(seed).randint(0, len - T).  The reference seeds the legacy GLOBAL generators with the first index it is
    asked for (kth.py:58-62): `seed` plays that role, and the private generators here produce the same streams."""

    def __init__(self, index, seq_len, seed):
        self.index, self.seq_len = index, seq_len
        self.np_rng, self.py_rng = np.random.RandomState(seed), random.Random(seed)
        self.bases, self.lengths = index.bases, index.lengths
        if not (self.lengths >= seq_len).any():
            raise SystemExit(f"dataset: no {index.dataset} {index.split} sequence has {seq_len} frames")

    def draw(self):
        """(pool index of the clip's first frame, label)."""
        vids = self.index.videos
        while True:                                     # skip sequences that are too short
            c = self.np_rng.randint(len(vids))
            v = self.np_rng.randint(len(vids[c]))
            s = vids[c][v][self.np_rng.randint(len(vids[c][v]))]
            if self.lengths[s] - self.seq_len >= 0:
                break
        st = self.py_rng.randint(0, int(self.lengths[s]) - self.seq_len)
        return int(self.bases[s]) + st, self.index.labels[s]

    def position(self):
        """Where both draw streams stand (data.BatchStream; train.py --resume)."""
        return {"sampler": "MetaSampler", "np": self.np_rng.get_state(), "py": self.py_rng.getstate()}

    def restore(self, pos):
        check_position(pos, "MetaSampler")
        self.np_rng.set_state(pos["np"])
        self.py_rng.setstate(pos["py"])


class BairSampler:
    """RobotPush.get_seq (bair.py:42-57): train draws np.random.randint(len(dirs)) from the generator seeded with the first
    index, test walks the directories in order and wraps; a clip always starts at frame 0.  No label: -1."""

    def __init__(self, index, seq_len, seed):
        self.index, self.seq_len = index, seq_len
        self.ordered = index.split == 'test'
        self.np_rng = np.random.RandomState(seed)
        self.bases, self.d = index.bases, 0
        short = np.nonzero(index.lengths < seq_len)[0]
        if short.size:
            d = os.path.dirname(index.sequences[short[0]][0]) if index.sequences[short[0]] else "an empty directory"
            raise SystemExit(f"dataset: {d!r} holds fewer than {seq_len} consecutive <i>.png frames")

    def draw(self):
        if self.ordered:
            d = self.d
            self.d = 0 if self.d == len(self.bases) - 1 else self.d + 1
        else:
            d = self.np_rng.randint(len(self.bases))
        return int(self.bases[d]), -1

    def position(self):
        """The next directory of the ordered walk and the state of the random one (data.BatchStream; train.py --resume)."""
        return {"sampler": "BairSampler", "ordered": self.ordered, "d": self.d, "np": self.np_rng.get_state()}

    def restore(self, pos):
        check_position(pos, "BairSampler")
        if bool(pos["ordered"]) != self.ordered or not 0 <= int(pos["d"]) < len(self.bases):
            raise SystemExit("data position: saved for another BAIR split or tree")
        self.d = int(pos["d"])
        self.np_rng.set_state(pos["np"])


class FramesSampler:
    """Clips of a `frames` tree.  Train: the clip is np.random.RandomState(seed).randint(n_clips), drawn again while the clip is
    shorter than seq_len; the start frame randint(0, len - T + 1) from the same generator.  Test: an ordered walk over the clips
    that are long enough, from frame 0, wrapping at the end (like BairSampler).  No label: -1."""

    def __init__(self, index, seq_len, seed):
        self.index, self.seq_len = index, seq_len
        self.ordered = index.split == 'test'
        self.np_rng = np.random.RandomState(seed)
        self.bases, self.lengths = index.bases, index.lengths
        self.long = np.nonzero(self.lengths >= seq_len)[0]      # the clips the ordered walk visits
        self.d = 0
        if not self.long.size:
            raise SystemExit(f"dataset: no frames {index.split} clip has {seq_len} frames")

    def draw(self):
        if self.ordered:
            s = int(self.long[self.d])
            self.d = 0 if self.d == len(self.long) - 1 else self.d + 1
            return int(self.bases[s]), -1
        while True:                                             # skip clips that are too short
            s = self.np_rng.randint(len(self.bases))
            if self.lengths[s] >= self.seq_len:
                break
        st = self.np_rng.randint(0, int(self.lengths[s]) - self.seq_len + 1)
        return int(self.bases[s]) + st, -1

    def position(self):
        """The next clip of the ordered walk and the state of the random one (data.BatchStream; train.py --resume)."""
        return {"sampler": "FramesSampler", "ordered": self.ordered, "d": self.d, "np": self.np_rng.get_state()}

    def restore(self, pos):
        check_position(pos, "FramesSampler")
        if bool(pos["ordered"]) != self.ordered or not 0 <= int(pos["d"]) < len(self.long):
            raise SystemExit("data position: saved for another frames split or tree")
        self.d = int(pos["d"])
        self.np_rng.set_state(pos["np"])


def check_position(pos, sampler):
    if not isinstance(pos, dict) or pos.get("sampler") != sampler:
        got = pos.get("sampler") if isinstance(pos, dict) else type(pos).__name__
        raise SystemExit(f"data position: saved for {got}, this run draws from {sampler}")


def make_sampler(index, seq_len, seed):
    return {'bair': BairSampler, 'frames': FramesSampler}.get(index.dataset, MetaSampler)(index, seq_len, seed)


# ---- --augment: per-clip augmentation parameters, drawn on the host, applied by ops.clip_gather_aug -----------------------------
AUGMENT_SEED_XOR = 0x5A17C11B   # data._clip_batches: the augmenter's seed = the generator's seed ^ this
MAX_SHIFT = 16                  # DVG_CLIP_MAX_SHIFT of dvg_amd/csrc/clips.hip
MAX_JITTER = 0.5


def parse_augment(spec):
    """'hflip,reverse,shift=N,jitter=G' (any subset, any order; N an integer in 1..16, 0 < G <= 0.5) ->
    {'hflip': bool, 'reverse': bool, 'shift': N or 0, 'jitter': G or 0.0}.  '' = no augmentation.  An unknown word, a duplicate
    or a value out of range ends the program naming it."""
    cfg = {'hflip': False, 'reverse': False, 'shift': 0, 'jitter': 0.0}
    seen = set()
    for word in [w.strip() for w in str(spec).split(',')] if str(spec).strip() else []:
        name, eq, value = word.partition('=')
        if name not in cfg or (name in ('hflip', 'reverse')) == bool(eq):
            raise SystemExit(f"--augment: unknown word {word!r} (hflip | reverse | shift=N | jitter=G)")
        if name in seen:
            raise SystemExit(f"--augment: {name!r} is given twice")
        seen.add(name)
        if name == 'shift':
            if not value.isdigit() or not 1 <= int(value) <= MAX_SHIFT:
                raise SystemExit(f"--augment: {word!r}: the shift is an integer in 1..{MAX_SHIFT}")
            cfg['shift'] = int(value)
        elif name == 'jitter':
            try:
                cfg['jitter'] = float(value)
            except ValueError:
                cfg['jitter'] = float('nan')
            if not 0.0 < cfg['jitter'] <= MAX_JITTER:           # a NaN, parsed or not a number at all, fails this as well
                raise SystemExit(f"--augment: {word!r}: the jitter is a number in (0, {MAX_JITTER}]")
        else:
            cfg[name] = True
    return cfg


def augment_spec(cfg):
    """The canonical spec string of a parsed one: the fixed order hflip, reverse, shift, jitter ('' = nothing enabled)."""
    words = [n for n in ('hflip', 'reverse') if cfg[n]]
    words += ['shift=%d' % cfg['shift']] if cfg['shift'] else []
    words += ['jitter=%s' % repr(float(cfg['jitter']))] if cfg['jitter'] else []
    return ','.join(words)


def add_arguments(p) -> None:
    """train.py's `--augment` option (as ema.add_arguments: the option lives with what it configures)."""
    p.add_argument('--augment', default='', metavar='LIST',   # docs/DESIGN_NOTES_augment.md
                   help='kth | bair | ucf | frames from --data_root, train split only: a comma list of hflip, reverse, shift=N (1..16 pixels, '
                        'edge-replicated) and jitter=G (0 < G <= 0.5: contrast and brightness); parameters are drawn per clip and '
                        'applied on the device inside the gather (default: none)')
    add_resize_arguments(p)


def add_resize_arguments(p) -> None:
    """`--resize` / `--resize_fit` of train.py and generate_frames.py (docs/DESIGN_NOTES_frames.md)."""
    # default=SUPPRESS: a run without the flags has the options object it always had (resize_spec supplies none / crop)
    p.add_argument('--resize', default=argparse.SUPPRESS, choices=('none',) + resample.FILTERS,
                   help='kth | bair | ucf | frames from --data_root: scale every decoded frame that is not image_width x image_width '
                        'with this filter of Pillow\'s Image.resize, on the device while the frame pool is built, bit-equal to '
                        'Pillow (default none: such a frame is refused)')
    p.add_argument('--resize_fit', default=argparse.SUPPRESS, choices=resample.FITS,
                   help='--resize: crop = the largest centred box of the target\'s aspect ratio, stretch = the whole frame (default crop)')


def resize_spec(opt):
    """(filter, fit) of an options object, None without `--resize` (objects made before the option existed have none)."""
    f = getattr(opt, 'resize', None) or 'none'
    fit = getattr(opt, 'resize_fit', None) or 'crop'
    if f != 'none' and f not in resample.FILTERS or fit not in resample.FITS:
        raise SystemExit(f"--resize {f} --resize_fit {fit}: none | {' | '.join(resample.FILTERS)} and {' | '.join(resample.FITS)}")
    return None if f == 'none' else (f, fit)


def check_resize(opt, who='train.py'):
    """`--resize` scales frames that are READ: refused, before anything is built, where no frame is (the choices are argparse's)."""
    spec = resize_spec(opt)
    if spec and (opt.dataset not in REAL_DATASETS or getattr(opt, 'synthetic_data', False)):
        raise SystemExit(f"{who} --resize: applies to kth | bair | ucf | frames clips read from --data_root, not to "
                         f"{'--synthetic_data' if getattr(opt, 'synthetic_data', False) else '--dataset ' + opt.dataset}")
    return spec


def check_augment(opt) -> str:
    """train.py: the canonical form of `--augment` ('' = off).  It augments clips that are gathered from a frame pool: the
    Moving-MNIST and synthetic streams draw a new clip for every batch, there is nothing to augment."""
    spec = augment_spec(parse_augment(opt.augment))
    if spec and (opt.dataset not in REAL_DATASETS or opt.synthetic_data):
        raise SystemExit(f"train.py --augment: applies to kth | bair | ucf | frames clips read from --data_root, not to "
                         f"{'--synthetic_data' if opt.synthetic_data else '--dataset ' + opt.dataset}")
    return spec


class ClipAugmenter:
    """The draws of `--augment`: one private np.random.RandomState(seed), apart from the samplers' generators, so the clips a
    run selects are the same with and without augmentation.  Per clip in batch order, and only for the enabled transforms, in
    this order: hflip = randint(2); reverse = randint(2); dy = randint(-N, N + 1), then dx; c = 1 + uniform(-G, G), then
    b = uniform(-G, G) / 2.  gain = float32(c), bias = float32(0.5 - 0.5 * c + b): contrast about mid-grey plus brightness,
    computed in float64 and rounded once.  Parameters are per CLIP, not per frame: the motion stays coherent."""

    def __init__(self, spec, seed):
        self.cfg = spec if isinstance(spec, dict) else parse_augment(spec)
        self.spec = augment_spec(self.cfg)
        self.rng = np.random.RandomState(seed)

    def draw(self, B):
        """(geom (B,4) int32 [hflip, reverse, dy, dx], photo (B,2) float32 [gain, bias]); disabled: 0, 0, 0, 0 and 1.0, 0.0."""
        cfg, rng = self.cfg, self.rng
        geom = np.zeros((B, 4), np.int32)
        photo = np.tile(np.array([1.0, 0.0], np.float32), (B, 1))
        N, G = cfg['shift'], cfg['jitter']
        for i in range(B):
            if cfg['hflip']:
                geom[i, 0] = rng.randint(2)
            if cfg['reverse']:
                geom[i, 1] = rng.randint(2)
            if N:
                geom[i, 2] = rng.randint(-N, N + 1)
                geom[i, 3] = rng.randint(-N, N + 1)
            if G:
                c = 1.0 + rng.uniform(-G, G)
                b = rng.uniform(-G, G) / 2.0
                photo[i, 0] = np.float32(c)
                photo[i, 1] = np.float32(0.5 - 0.5 * c + b)
        return geom, photo

    def position(self):
        return {"spec": self.spec, "np": self.rng.get_state()}

    def restore(self, pos):
        got = pos.get("spec") if isinstance(pos, dict) else None
        if got != self.spec:
            raise SystemExit(f"data position: saved with --augment {got!r}, this run has --augment {self.spec!r}")
        self.rng.set_state(pos["np"])


def _decode(path, dst, image_width, resize=None):
    """One PNG into dst (H,W,pool_c) uint8: mode L as one channel, RGB interleaved; no resizing (nor does the reference) unless
    `resize` = (filter, fit) is given: a frame of another size is then scaled by Pillow itself, here on the decoding thread (the
    host pool; what the device path must equal byte for byte)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.size != (image_width, image_width) and resize is None:
                raise SystemExit(f"dataset: {path!r} is {im.size[0]}x{im.size[1]}, not {image_width}x{image_width}"
                                 f" (--resize FILTER scales such frames)")
            if im.mode != ('L' if dst.shape[2] == 1 else 'RGB'):
                raise SystemExit(f"dataset: {path!r} has mode {im.mode}, the pool holds {dst.shape[2]}-channel frames")
            if im.size != (image_width, image_width):
                im = resample.pil_resize(im, image_width, *resize)
            dst[...] = np.asarray(im).reshape(dst.shape)
    except OSError as e:
        raise SystemExit(f"dataset: cannot read {path!r}: {e}")


def _frame_size(path):
    """(W, H) from the file's header."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            return im.size
    except OSError as e:
        raise SystemExit(f"dataset: cannot read {path!r}: {e}")


def _decode_native(path, dst):
    """One frame at its own size into dst (H,W,pool_c) uint8 (a view of the staging buffer)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode != ('L' if dst.shape[2] == 1 else 'RGB'):
                raise SystemExit(f"dataset: {path!r} has mode {im.mode}, the pool holds {dst.shape[2]}-channel frames")
            if im.size != (dst.shape[1], dst.shape[0]):
                raise SystemExit(f"dataset: {path!r} changed its size while it was read")
            dst[...] = np.asarray(im).reshape(dst.shape)
    except OSError as e:
        raise SystemExit(f"dataset: cannot read {path!r}: {e}")


def _pool_channels(path):
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode not in ('L', 'RGB'):
                raise SystemExit(f"dataset: {path!r} has mode {im.mode}: only L and RGB PNGs are read")
            return 1 if im.mode == 'L' else 3
    except OSError as e:
        raise SystemExit(f"dataset: cannot read {path!r}: {e}")


_pools = {}     # (dataset, root, split, width, device, resize) -> the pool build_pool made: the streams of one split share it


def shared_pool(index, root, image_width, device=None, threads=5, resize=None):
    """build_pool(index, ...), once per (dataset, root, split, width, device, resize) and process: train.py's test stream and
    its validation stream (--val_every) read the test split from ONE frame pool.  The pool is read only."""
    dev = torch.device(device) if device is not None else torch.device('cpu')
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (index.dataset, os.path.abspath(root), index.split, int(image_width), str(dev), None if resize is None else tuple(resize))
    if key not in _pools:
        _pools[key] = build_pool(index, image_width, dev, threads, resize)
    return _pools[key]


def build_pool(index, image_width, device=None, threads=5, resize=None):
    """(n_frames, S, S, pool_c) uint8: every frame of `index`, sequence after sequence (sequence i starts at index.bases[i]).
    Decoded with Pillow on min(threads, 16) threads.  For a GPU `device` the frames are decoded into a pinned staging
    buffer of at most STAGING_BYTES and uploaded chunk by chunk into ONE device tensor; device None / cpu: a host tensor.
    resize = (filter, fit) (`--resize`, `--resize_fit`): frames of another size are scaled to S x S as Pillow's Image.resize
    scales them - for a GPU device by dvg_resample_u8 (_build_pool_resized), for a host pool by Pillow on the decoding thread;
    the two pools are equal byte for byte.  None: such a frame ends the program, and nothing here differs from before."""
    files = [f for seq in index.sequences for f in seq]
    if not files:
        raise SystemExit(f"dataset: the {index.dataset} {index.split} split lists no frame")
    pc = _pool_channels(files[0])
    frame_bytes = image_width * image_width * pc
    dev = torch.device(device) if device is not None else torch.device('cpu')
    pool = torch.empty((len(files), image_width, image_width, pc), dtype=torch.uint8, device=dev)
    workers = max(1, min(int(threads), MAX_DECODE_THREADS))
    with ThreadPoolExecutor(workers) as ex:
        if dev.type == 'cpu':
            host = pool.numpy()
            list(ex.map(lambda i: _decode(files[i], host[i], image_width, resize), range(len(files))))
            return pool
        if resize is not None:
            return _build_pool_resized(ex, files, pool, resize)
        chunk = max(1, min(len(files), STAGING_BYTES // frame_bytes))
        staging = torch.empty((chunk, image_width, image_width, pc), dtype=torch.uint8).pin_memory()
        host = staging.numpy()
        for a in range(0, len(files), chunk):
            n = min(chunk, len(files) - a)
            list(ex.map(lambda i: _decode(files[a + i], host[i], image_width), range(n)))
            pool[a:a + n].copy_(staging[:n], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()      # the staging buffer is written again by the next chunk
    return pool


def _build_pool_resized(ex, files, pool, resize):
    """build_pool's GPU path under `--resize`: the worker threads decode every frame at its OWN size into the pinned staging
    buffer, packed by bytes (at most STAGING_BYTES a chunk; a run of equal-sized frames starts 16-byte aligned and is contiguous);
    each run of consecutive frames with the same (H, W) is then one upload and one ops.resample_u8 straight into its slice of
    the pool (a run that already is S x S: one copy).  The sizes come from the files' headers first, so the packing is known
    before a pixel is decoded."""
    from . import ops
    dev, S, pc = pool.device, pool.shape[1], pool.shape[3]
    flt, fit = resize
    sizes = list(ex.map(_frame_size, files))                      # (W, H)
    nbytes = [w * h * pc for w, h in sizes]
    cap = max(min(STAGING_BYTES, sum(nbytes) + 16 * len(files)), max(nbytes))
    staging = torch.empty(cap, dtype=torch.uint8).pin_memory()
    landing = torch.empty(cap, dtype=torch.uint8, device=dev)
    host = staging.numpy()
    a = 0
    while a < len(files):
        offs, used, b = [], 0, a
        while b < len(files):
            at = used if b > a and sizes[b] == sizes[b - 1] else (used + 15) & ~15
            if b > a and at + nbytes[b] > cap:
                break
            offs.append(at)
            used = at + nbytes[b]
            b += 1

        def decode(i):
            w, h = sizes[a + i]
            _decode_native(files[a + i], host[offs[i]:offs[i] + nbytes[a + i]].reshape(h, w, pc))
        list(ex.map(decode, range(b - a)))
        i = a
        while i < b:
            j = i + 1
            while j < b and sizes[j] == sizes[i]:
                j += 1
            (w, h), o0, o1 = sizes[i], offs[i - a], offs[i - a] + (j - i) * nbytes[i]
            landing[o0:o1].copy_(staging[o0:o1], non_blocking=True)
            src = landing[o0:o1].view(j - i, h, w, pc)
            if (w, h) == (S, S):
                pool[i:j].copy_(src)
            else:
                ops.resample_u8(src, (S, S), flt, box=resample.fit_box(w, h, S, S, fit), out=pool[i:j])
            i = j
        torch.cuda.current_stream(dev).synchronize()              # the staging buffer is written again by the next chunk
        a = b
    return pool
