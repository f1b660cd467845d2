"""dvg_convT4x4s2_bn_act_proj without a GPU: every precondition of the fused launch is checked on the host and fails BEFORE
anything is launched (no fall-through to another kernel), and fused.py offers the path only for shapes the entry point takes."""
import pytest
import torch


def _call(**kw):
    from dvg_amd import _lib
    a = dict(x=64, w=64, scale=0, shift=0, proj_w=64, proj_out=64, T=9, N=2, H=8, W=8, C1=64, Cout=64, act=1, slope=0.2,
             addend=0, addend_map=0, addend_block=0)     # pointers: aligned non-NULL stand-ins, never dereferenced by a failing call
    a.update(kw)
    lib = _lib.lib()
    code = lib.dvg_convT4x4s2_bn_act_proj(a["x"] or None, a["w"] or None, a["scale"] or None, a["shift"] or None,
                                          a["proj_w"] or None, a["proj_out"] or None, a["T"], a["N"], a["H"], a["W"], a["C1"],
                                          a["Cout"], a["act"], a["slope"], a["addend"] or None, a["addend_map"] or None,
                                          a["addend_block"], None)
    return code, lib.dvg_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(Cout=128), "Cout=128 must be 64"),
    (dict(T=0), "T=0"),
    (dict(T=49), "T=49"),
    (dict(proj_out=0), "NULL"),
    (dict(proj_w=0), "NULL"),
    (dict(proj_w=68), "aligned"),
    (dict(C1=24), "C1=24"),
    (dict(H=4, W=4), "unsupported map"),          # the 4 x 4 x 4-image tile has no projecting instantiation
    (dict(H=12), "unsupported map"),
    (dict(addend=64, addend_map=64, addend_block=3), "addend_block"),
    (dict(act=7), "bad act"),
])
def test_failed_precondition_is_an_error_before_the_launch(kw, word):
    code, msg = _call(**kw)
    assert code != 0 and word in msg and "dvg_convT4x4s2_bn_act_proj" in msg, (code, msg)


def test_fused_path_is_offered_only_where_the_entry_point_applies():
    from dvg_amd import fused
    conv = torch.nn.Conv2d(128, 64, 3, 1, 1)
    x = torch.zeros(1, 64, 32, 32)
    ok = torch.nn.ConvTranspose2d(64, 1, 3, 1, 1)
    with torch.no_grad():
        assert fused.LAST_PROJ_FUSED and fused._last_proj_applies(ok, conv, x)
        assert fused._last_proj_applies(torch.nn.ConvTranspose2d(64, 5, 3, 1, 1), conv, x)          # T = 45
        assert not fused._last_proj_applies(torch.nn.ConvTranspose2d(64, 6, 3, 1, 1), conv, x)      # T = 54 > 48
        assert not fused._last_proj_applies(torch.nn.ConvTranspose2d(64, 1, 4, 2, 1), conv, x)      # dcgan's last layer
        assert not fused._last_proj_applies(None, conv, x)
        assert not fused._last_proj_applies(ok, torch.nn.Conv2d(256, 128, 3, 1, 1), x)              # Cout = 128
        assert not fused._last_proj_applies(ok, conv, torch.zeros(1, 64, 4, 4))                     # the 4 x 4 tile
    assert not fused._last_proj_applies(ok, conv, x)                                                # grad mode
