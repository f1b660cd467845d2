#!/usr/bin/env python3
"""Writes tests/golden/reference_viz.npz: outputs of the REFERENCE's own utils.image_tensor and utils.draw_text_tensor.

Run in the build container only (needs the reference tree, CPU is enough; Pillow for draw_text_tensor):

    python tests/golden/make_golden_viz.py [path of the reference, default: the one make_golden.py uses]

The reference's utils.py imports skimage, imageio, torchvision, sklearn and scipy.misc at module level, none of which its
image_tensor / draw_text_tensor use; whichever of them cannot be imported here is replaced by an empty stand-in module
BEFORE the import.  The inputs are regenerated from seeds (tests/viz_ref.py: golden_inputs, golden_text_frame), so the file
holds outputs only: data, never reference source.  add_border and the figure assemblies live in scripts that execute on
import and are restated in tests/viz_ref.py instead."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"          # as in make_golden.py

STUBBED = ("sklearn", "sklearn.manifold", "scipy.misc", "matplotlib", "matplotlib.pyplot", "skimage", "skimage.measure",
           "torchvision", "imageio")


def stub_missing():
    for name in STUBBED:
        try:
            importlib.import_module(name)
        except Exception:
            m = types.ModuleType(name)
            m.__getattr__ = lambda attr: (lambda *a, **k: None)    # `from x import y` of anything succeeds
            m.__path__ = []
            sys.modules[name] = m
            parent, _, child = name.rpartition(".")
            if parent and parent in sys.modules:
                setattr(sys.modules[parent], child, m)


def reference_utils(ref):
    stub_missing()
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(ref, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from tests import viz_ref
    ref = reference_utils(sys.argv[1] if len(sys.argv) > 1 else REF)
    out = {}
    for name in viz_ref.GOLDEN_CASES:
        inputs, padding = viz_ref.golden_inputs(name)
        out[name] = ref.image_tensor(inputs, padding).numpy()
    out["draw_text_empty"] = ref.draw_text_tensor(viz_ref.golden_text_frame(), "").numpy()
    path = os.path.join(HERE, "reference_viz.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
