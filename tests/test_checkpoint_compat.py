"""CPU: a checkpoint pickled by the REFERENCE (whole nn.Module objects, train.py:380-383) must unpickle into our
classes through the top-level `models` alias package, with an identical attribute tree.  Fixture:
tests/golden/reference_pickled_modules.pth.gz, written by tests/golden/make_golden.py from the reference's own classes
(torch.manual_seed(0), default init; every tensor zeroed but the one compared here, whose SHA-256 was taken before pickling)."""
import gzip
import hashlib
import importlib
import io
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_pickled_modules.pth.gz")


def _load_fixture():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    raw = gzip.open(FIXTURE).read()
    return torch.load(io.BytesIO(raw), weights_only=False)   # resolves models.<name> -> our alias package


@pytest.mark.parametrize("name", ["dcgan_64", "vgg_64"])
def test_reference_pickle_loads_into_our_classes(name):
    ck = _load_fixture()[name]
    ours = importlib.import_module(f"dvg_amd.models.{name}")
    enc, dec = ck["modules"]["encoder"], ck["modules"]["decoder"]
    assert isinstance(enc, ours.encoder) and isinstance(dec, ours.decoder)
    assert list(enc.state_dict().keys()) == ck["encoder_keys"]
    assert list(dec.state_dict().keys()) == ck["decoder_keys"]
    key = "c2.main.0.weight" if name == "dcgan_64" else "c2.0.main.0.weight"
    assert ck["weight_key"] == key
    w = enc.state_dict()[key]
    assert float(w.abs().max()) > 0
    assert hashlib.sha256(w.contiguous().numpy().tobytes()).hexdigest() == ck["weight_sha256"]
    # the unpickled object has OUR forward (HIP path): calling it on CPU must refuse, not silently run torch.nn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 1, 64, 64))
    # layer wrappers are our classes too (the decoder walks isinstance(layer, vgg_layer))
    if name == "vgg_64":
        assert isinstance(dec.upc2[0], ours.vgg_layer)
