"""Shared helpers for the parity tests (regenerate the seeded weights/inputs of make_golden.py)."""
import importlib
import os
import re

import torch

from oracle import dvg_oracle as orc
from oracle import params

# tag -> (family, res, nc, batch, training, seed)   — must mirror tests/golden/make_golden.py:main()
BACKBONE_CASES = {
    "vgg_64/eval": ("vgg", 64, 1, 2, False, 100),
    "vgg_64/train": ("vgg", 64, 1, 4, True, 110),
    "dcgan_64/eval": ("dcgan", 64, 1, 2, False, 120),
    "dcgan_64/train": ("dcgan", 64, 1, 4, True, 130),
    "vgg_64_nc3/eval": ("vgg", 64, 3, 2, False, 140),
    "dcgan_64_nc3/eval": ("dcgan", 64, 3, 2, False, 150),
    "vgg_128/eval": ("vgg", 128, 3, 1, False, 160),
    "dcgan_128/eval": ("dcgan", 128, 3, 2, False, 170),
}


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    """include/dvg_hip.h without its comments: what the host tests read the C ABI from (one place; shares no code with the
    parser of dvg_amd/_lib.py, which tests/test_abi.py holds to it)."""
    with open(os.path.join(ROOT, "include", "dvg_hip.h")) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(dvg_[a-zA-Z0-9_]+)\s*\(", header_text())))


def header_declaration(name):
    """(return type, [parameters]) of an entry point as the header spells them, whitespace collapsed; `(void)` gives []."""
    m = re.search(rf"(?:^|[;{{\n])\s*([A-Za-z_][\w\s*]*?)\s*\b{name}\s*\(([^()]*)\)\s*;", header_text())
    assert m, f"{name} is not declared in include/dvg_hip.h"
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return " ".join(m.group(1).split()), [] if params == ["void"] else params


def dev():
    """The device of the GPU tests (they are all marked `gpu`: run on the MI355X box only)."""
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nhwc(t):
    from dvg_amd import ops
    return ops.to_nhwc(t.to(dev()))


def our_module(family, res):
    return importlib.import_module(f"dvg_amd.models.{family}_{res}")


def backbone_case(tag):
    """Returns (enc_module, dec_module, enc_sd, dec_sd, x, vec) for a golden case, modules on CPU."""
    family, res, nc, batch, training, seed = BACKBONE_CASES[tag]
    mod = our_module(family, res)
    enc, dec = mod.encoder(90, nc), mod.decoder(90, nc)
    esd = params.fill_state_dict(enc.state_dict(), seed)
    dsd = params.fill_state_dict(dec.state_dict(), seed + 1, params.decoder_transposed_keys(dec.state_dict(), family))
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    enc.train(training)
    dec.train(training)
    x = params.frames(seed + 2, batch, nc, res)
    vec = params.normal(seed + 3, batch, 90, scale=0.5).tanh()
    return enc, dec, esd, dsd, x, vec


def oracle_backbone(tag, esd, dsd, x, vec):
    """Oracle forward for a case; mutates copies of the state dicts in train mode (running stats)."""
    family, res, nc, batch, training, seed = BACKBONE_CASES[tag]
    esd = {k: v.clone() for k, v in esd.items()}
    dsd = {k: v.clone() for k, v in dsd.items()}
    if family == "vgg":
        h, skips = orc.vgg_encoder(x, esd, training)
        y = orc.vgg_decoder(vec, skips, dsd, training)
        y_h = orc.vgg_decoder(h, skips, dsd, training)
    else:
        act = "tanh" if res == 64 else "sigmoid"
        h, skips = orc.dcgan_encoder(x, esd, training)
        y = orc.dcgan_decoder(vec, skips, dsd, training, act)
        y_h = orc.dcgan_decoder(h, skips, dsd, training, act)
    return h, skips, y, y_h, esd, dsd


def summarize(t: torch.Tensor, k: int = 64):
    f = t.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, f.numel() - 1, k).long()
    return torch.cat([torch.stack([f.sum(), f.abs().sum(), (f * f).sum()]), f[idx]]).numpy()


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a-b| / max |b|: the largest ABSOLUTE deviation relative to the tensor's largest magnitude - a GLOBAL (tensor-wide)
    relative error, not an element-wise one.  This is the figure every "1e-4 relative" claim of this repository refers to
    (BASELINE.json's bar is stated on fp32 frames, whose values fill [0, 1] / [-1, 1], so tensor-wide and element-wise
    agree there up to the frames' dynamic range); for latents in (-1, 1) with entries near 0 it is the more generous of the
    two, which is why the latent checks that matter (GP moments, LSTM outputs) also carry absolute bars.  `rel_err_elem`
    below is the element-wise figure."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def rel_err_elem(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-2) -> float:
    """max over elements of |a-b| / max(|b|, floor * max |b|): element-wise relative error with a floor at `floor` of the
    tensor's largest magnitude (an entry that is ~0 by cancellation has no meaningful relative error)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.abs().clamp_min(floor * max(float(b.abs().max()), 1e-12))
    return float(((a - b).abs() / den).max())


class record_hip_kinks:
    """`with record_hip_kinks(enc, dec) as acts:` records, from the HIP training-path forward of these modules, the OUTPUT of
    every conv + BatchNorm + LeakyReLU block and of the decoder stem under the oracle's layer prefix ("c1.0", "upc2.1",
    "upc1" ...): what oracle.forced_kinks consumes to take the same LeakyReLU / max-pool branches as the kernels did
    (backward.hip decides both from the saved output y: `y > 0`, first maximum of the 2x2 window in scan order).
    Recording wraps dvg_amd.autograd.conv_block_autograd / dense_block_autograd, the two functions every train-mode block goes
    through; a module called more than once keeps a list (call order)."""

    def __init__(self, *modules):
        self.names = {}
        for m in modules:
            for name, sub in m.named_modules():
                if name.endswith(".main.0"):
                    self.names[id(sub)] = name[:-len(".main.0")]
                elif name == "upc1.0":
                    self.names[id(sub)] = "upc1"

    def __enter__(self):
        from dvg_amd import autograd as ag
        self.ag, self.orig = ag, (ag.conv_block_autograd, ag.dense_block_autograd)
        self.acts = {}

        def keep(conv, out):
            name = self.names.get(id(conv))
            if name is not None:
                y = out[0] if isinstance(out, tuple) else out
                self.acts.setdefault(name, []).append(y.detach().cpu().contiguous())

        def conv_block(kind, conv, bn, x, skip, **kw):
            out = self.orig[0](kind, conv, bn, x, skip, **kw)
            keep(conv, out)
            return out

        def dense_block(kind, conv, bn, x, **kw):
            out = self.orig[1](kind, conv, bn, x, **kw)
            if kind == "stem":
                keep(conv, out)
            return out
        ag.conv_block_autograd, ag.dense_block_autograd = conv_block, dense_block
        return self.acts

    def __exit__(self, *exc):
        self.ag.conv_block_autograd, self.ag.dense_block_autograd = self.orig


def single_call_kinks(acts):
    """acts of record_hip_kinks when every module ran once: prefix -> tensor."""
    assert all(len(v) == 1 for v in acts.values()), {k: len(v) for k, v in acts.items() if len(v) != 1}
    return {k: v[0] for k, v in acts.items()}


# The fp64 yardstick runs of the oracle at the reference's batch sizes (B = 50: minutes of host time) are opt-in: every bar they
# produced is at or below 1e-4 now and recorded in DESIGN.md 4 / profiles/r05_yardsticks.txt; DVG_TEST_YARDSTICK=1 re-measures.
# The small-batch yardsticks (B = 4 ... 16) always run.
import os as _os
YARDSTICK_AT_SCALE = _os.environ.get("DVG_TEST_YARDSTICK") == "1"


def to64(obj):
    """A tensor / state dict / list of tensors in float64 (integer entries - num_batches_tracked - unchanged)."""
    if torch.is_tensor(obj):
        return obj.double() if obj.is_floating_point() else obj.clone()
    if isinstance(obj, dict):
        return {k: to64(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to64(v) for v in obj)
    return obj


def _err(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return rel_err(a, b)
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def yardstick(name, hip, ref32, ref64, *, ratio=1.5, slack=0.0):
    """The fp64 yardstick of the GP tests for every parity bar above 1e-4: the oracle's arithmetic in fp64 is the
    truth, the oracle's own fp32 run (torch-CPU: the reference's arithmetic) shows how far fp32 rounding alone moves the
    quantity - train-mode BatchNorm divides by batch statistics and amplifies it - and the HIP result must not be further from
    the truth than `ratio` x that (+ `slack`, an absolute rel-err allowance where the fp32 oracle happens to land within a few
    ulps).  Prints all three; returns (HIP error, fp32-oracle error), both against fp64."""
    e_hip, e_32, e_pair = _err(hip, ref64), _err(ref32, ref64), _err(hip, ref32)
    print(f"yardstick {name}: HIP vs fp64 oracle {e_hip:.2e} | fp32 oracle vs fp64 oracle {e_32:.2e} | HIP vs fp32 oracle "
          f"{e_pair:.2e} | ratio {e_hip / max(e_32, 1e-30):.2f}")
    assert e_hip <= ratio * e_32 + slack, (name, e_hip, e_32, ratio)
    return e_hip, e_32
