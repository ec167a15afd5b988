"""What a supersampled render must produce, built from the oracle alone (tests/test_supersampling_gpu.py): the oracle's
s*W x s*H frame in the plain fp32 x 3 format, the s*s samples of a pixel summed in fp32 one after the other in row-major
order, divided by float(s*s), and packed by the oracle's own pack_pixel."""
import ctypes as C

import numpy as np

import fixtures as fx
import oracle_binding as ob
import support as sup


def mean_colors(osc, w, h, s):
    """(h, w, 3) float32: the box-filtered colours of the oracle scene's s*w x s*h frame"""
    hi = osc.render(s * w, s * h, fx.RGBF32, threads=sup.worker_threads()).view(">f4").astype(np.float32).reshape(s * h, s * w, 3)
    acc = hi[0::s, 0::s]
    for j in range(s):
        for i in range(s):
            if i == 0 and j == 0:
                continue
            acc = (acc + hi[j::s, i::s]).astype(np.float32)
    return (acc / np.float32(s * s)).astype(np.float32)


def pack(mean, channels, reversed_=False):
    """(h, w * bpp) uint8: every colour of `mean` through the oracle's pack_pixel"""
    ch, bpp = ob.make_channels(channels)
    mean = np.ascontiguousarray(mean, np.float32)
    h, w = mean.shape[:2]
    out = np.zeros((h, w * bpp), np.uint8)
    fn = ob.lib().nto_pack_pixel
    src, dst = mean.ctypes.data, out.ctypes.data
    nch, rev = len(ch), int(bool(reversed_))
    for k in range(h * w):
        fn(C.cast(src + 12 * k, ob.f32p), nch, ch, rev, bpp, C.cast(dst + bpp * k, C.POINTER(C.c_uint8)))
    return out


def expected(osc, w, h, s, channels, reversed_=False):
    return pack(mean_colors(osc, w, h, s), channels, reversed_)
