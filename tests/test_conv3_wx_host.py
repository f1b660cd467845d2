"""CPU: the WX form of the direct 3x3 conv (1-D Winograd F(2,3) along x inside the kernel, conv_igemm2.hip: conv3_wx_kernel).

  * the algebra: for random fp64 d and g the four products per pair and kernel row, summed over the three kernel rows and put
    through the output transform, are the 3x3 conv (1e-12), and swapping v1 / v2 is not;
  * `pack_wx_numpy`, the numpy restatement of dvg_pack_conv_weight_wx's memory image (tests/test_gpu_conv3_wx.py compares the
    device packer with it bit for bit): the three bf16 planes of a row sum to the fp32 u_f exactly, tap = 4 r + f, the two
    16-byte halves of a plane swapped on rows with bit 3 set;
  * every host precondition of the three entry points returns its error before anything is launched (no GPU here)."""
import ctypes

import numpy as np
import pytest

from tests.test_bf16x3_split import split3


def wx_u(g):
    """u[..., r, f] of kernel rows g[..., r, 0..2], in g's dtype with the packer's order of operations."""
    half = g.dtype.type(0.5)
    return np.stack([g[..., 0], ((g[..., 0] + g[..., 1]) + g[..., 2]) * half, ((g[..., 0] - g[..., 1]) + g[..., 2]) * half,
                     g[..., 2]], axis=-1)


def wx_conv(x, w, swap_v12=False):
    """3x3 conv, padding 1, of x (N, C, H, W) with w (Co, C, 3, 3) in the kernel's F(2,3)-row form, in x's dtype.  swap_v12: the
    planted defect of the GPU test (v1 and v2 exchanged)."""
    n, c, h, wd = x.shape
    d = np.zeros((n, c, h + 2, wd + 2), x.dtype)
    d[:, :, 1:-1, 1:-1] = x
    u = wx_u(w)                                                    # (Co, C, r, f)
    y = np.zeros((n, w.shape[0], h, wd), x.dtype)
    for r in range(3):
        rows = d[:, :, r:r + h]                                    # halo row y + r of output row y
        e0, o0, e1, o1 = rows[..., 0:-2:2], rows[..., 1:-1:2], rows[..., 2::2], rows[..., 3::2]      # d[2j], d[2j+1], d[2j+2], d[2j+3]
        v = [e0 - e1, o0 + e1, e1 - o0, o0 - o1]
        if swap_v12:
            v[1], v[2] = v[2], v[1]
        m = [np.einsum("nchj,oc->nohj", v[f], u[:, :, r, f]) for f in range(4)]
        y[..., 0::2] += m[0] + m[1] + m[2]
        y[..., 1::2] += m[1] - m[2] - m[3]
    return y


def direct_conv(x, w):
    n, c, h, wd = x.shape
    d = np.zeros((n, c, h + 2, wd + 2), x.dtype)
    d[:, :, 1:-1, 1:-1] = x
    y = np.zeros((n, w.shape[0], h, wd), x.dtype)
    for a in range(3):
        for b in range(3):
            y += np.einsum("nchw,oc->nohw", d[:, :, a:a + h, b:b + wd], w[:, :, a, b])
    return y


def pack_wx_numpy(w):
    """Memory image of dvg_pack_conv_weight_wx (bf16-triple build) as uint16 [Cin/16][Cout/64][12][64][3 planes][16]."""
    w = np.asarray(w, np.float32)
    co, ci = w.shape[:2]
    u = wx_u(w)                                                    # fp32, (Co, Ci, r, f)
    planes = np.stack(split3(u), axis=-1)                          # (Co, Ci, r, f, plane) as fp32 holding bf16 values
    bits = (planes.view(np.uint32) >> 16).astype(np.uint16)
    out = np.zeros((ci // 16, co // 64, 12, 64, 3, 16), np.uint16)
    for c in range(co):
        for k in range(16):
            pos = (((k >> 3) ^ ((c >> 3) & 1)) << 3) + (k & 7)
            # (chunk, r, f, plane) of channel c, k-value k  ->  [chunk][block][4 r + f][c % 64][plane][pos]
            out[:, c // 64, :, c % 64, :, pos] = bits[c, k::16].reshape(ci // 16, 12, 3)
    return out


def test_f23_rows_summed_over_the_kernel_rows_are_the_conv():
    rng = np.random.default_rng(7100)
    x = rng.standard_normal((2, 5, 8, 16))
    w = rng.standard_normal((3, 5, 3, 3))
    ref = direct_conv(x, w)
    assert np.abs(wx_conv(x, w) - ref).max() <= 1e-12
    assert np.abs(wx_conv(x, w, swap_v12=True) - ref).max() > 1e-2      # the planted defect is a different function


def test_packed_rows_hold_the_exact_triples_of_u_in_tap_order():
    rng = np.random.default_rng(7101)
    w = (rng.standard_normal((128, 32, 3, 3)) / 17).astype(np.float32)
    img = pack_wx_numpy(w)
    assert img.shape == (2, 2, 12, 64, 3, 16)
    vals = (img.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    u = wx_u(w)
    assert u.dtype == np.float32
    for c in (0, 7, 8, 63, 64, 77, 127):
        for k in (0, 7, 8, 15):
            pos = (((k >> 3) ^ ((c >> 3) & 1)) << 3) + (k & 7)
            for chunk in range(2):
                got = vals[chunk, c // 64, :, c % 64, :, pos].sum(-1)                  # h + m + l, exact in fp64
                assert np.array_equal(got, u[c, chunk * 16 + k].reshape(12).astype(np.float64)), (c, k, chunk)
    # rows with bit 3 clear are not swapped: k-value 0 sits at position 0 of its plane
    assert np.array_equal(vals[0, 0, 0, 0, :, 0].sum(-1), np.float64(w[0, 0, 0, 0]))
    # u1 + u2 = g0 + g2 and u1 - u2 = g1 up to the fp32 roundings of the packer
    assert np.abs((u[..., 1] - u[..., 2]) - w[..., 1]).max() <= 4 * np.finfo(np.float32).eps * np.abs(w).max()


@pytest.fixture(scope="module")
def entry():
    from dvg_amd._lib import CONSTANTS, lib
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) & ~63
    return lib(), CONSTANTS, base, buf


def test_every_host_precondition_returns_its_error(entry):
    lib, K, base, _keep = entry
    SHAPE, NULL, ALIGN = K["ERR_SHAPE"], K["ERR_NULL"], K["ERR_ALIGN"]
    ptr = lambda off=0: ctypes.c_void_p(base + off)   # noqa: E731  never dereferenced: every call fails before its launch

    def pack(w=ptr(), out=ptr(), cout=64, cin=16):
        return lib.dvg_pack_conv_weight_wx(w, out, cout, cin, None)
    assert pack(w=None) == NULL and pack(out=None) == NULL
    assert pack(cout=32) == SHAPE and pack(cin=8) == SHAPE and pack(cout=0) == SHAPE
    assert pack(out=ptr(4)) == ALIGN

    def conv(x=ptr(), skip=None, w=ptr(), y=ptr(), yp=None, N=1, H=8, W=16, C1=16, C2=0, Cout=64, up=0, act=1, addend=None,
             amap=None, ablk=0):
        return lib.dvg_conv3x3_bn_act_wx(x, skip, w, None, None, y, yp, N, H, W, C1, C2, Cout, up, act, 0.2, addend, amap, ablk, None)
    assert conv(x=None) == NULL and conv(w=None) == NULL and conv(y=None) == NULL
    assert conv(C1=8) == SHAPE and conv(C1=24) == SHAPE                   # Cin % 16
    assert conv(Cout=32) == SHAPE and conv(Cout=96) == SHAPE              # Cout % 64
    assert conv(W=8) == SHAPE and conv(W=24) == SHAPE                     # W % 16
    assert conv(H=4) == SHAPE and conv(H=12) == SHAPE                     # H % 8
    assert conv(N=0) == SHAPE and conv(act=9) == SHAPE
    assert conv(C2=16, skip=ptr()) == SHAPE and conv(up=1) == SHAPE       # no concat operand, no upsampling
    assert conv(addend=ptr(), yp=ptr()) == SHAPE                          # the addend excludes the pooled output
    assert conv(addend=ptr(), amap=ptr(), ablk=0) == SHAPE and conv(N=3, addend=ptr(), amap=ptr(), ablk=2) == SHAPE
    for k in ("x", "w", "y", "yp", "addend"):
        assert conv(**{k: ptr(4)}) == ALIGN, k

    def first(frame=ptr(), w0=ptr(), s0=ptr(), h0=ptr(), w1=ptr(), y=ptr(), yp=ptr(), N=2, H=8, W=16, Cout=64, act=1, y_from=0):
        return lib.dvg_conv3x3_first_pair_wx(frame, w0, s0, h0, w1, None, None, y, yp, N, H, W, Cout, act, 0.2, y_from, None)
    for k in ("frame", "w0", "s0", "h0", "w1"):
        assert first(**{k: None}) == NULL, k
    assert first(y_from=-1) == SHAPE and first(y_from=3) == SHAPE
    assert first(y_from=1, yp=None) == SHAPE and first(y=None, y_from=1) == SHAPE
    assert first(Cout=32) == SHAPE and first(W=8) == SHAPE and first(H=12) == SHAPE and first(N=0) == SHAPE
    for k in ("frame", "w0", "w1", "y", "yp"):
        assert first(**{k: ptr(4)}) == ALIGN, k
    assert b"16-byte" in lib.dvg_last_error()
