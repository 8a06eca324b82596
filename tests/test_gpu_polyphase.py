"""The two integer polyphase kernels on the device (`pytest -m gpu`; DESIGN.md sections 15 and 16): at integer ratios resize_kernel_codes (imageProcess.resampleChroma)
and resize_kernel_fit (imageProcess.fitPlanes) are one filter and give the same bytes.  Both run polyphase.h's arithmetic from tables of their own (phase tables in the
kernel's arguments, per-output tables in device memory) under tiles of their own (256 x 32, 128 x 32 / 16 / 8): the planes below cross both tiles in both axes."""
import numpy as np
import pytest
import torch

from moephoto_amd import pixfmt

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 16: 'yuv420p16le'}
METHODS = ('nearest', 'bilinear', 'bicubic')
LOCS = ('center', 'left')
PAIRS = ((10, 8), (8, 16), (16, 10))
PLANES = (((33, 257), 1), ((11, 86), 3), ((9, 65), 4))          # ((h, w) of a chroma plane, scale): 33 x 257, 33 x 258 and 36 x 260 samples out


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _codes(seed, depth, h, w):
    """tests/test_gpu_chroma.py's planes: random codes of the container, 10-bit planes also with bit 15 set and one 65535 (high bits are not masked on input)."""
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=(2, h, w))
    if depth == 10:
        c.reshape(-1)[1::5] |= 0x8000
        c.reshape(-1)[2] = 65535
    return c.astype(np.uint8 if depth == 8 else '<u2')


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_resamplechroma_and_fitplanes_give_the_same_bytes_at_integer_ratios(method, loc, dev):
    from moephoto_amd import imageProcess as ip
    for (h, w), scale in PLANES:
        for ds, dd in PAIRS:
            C = _codes(h + scale + ds, ds, h, w)
            codes = torch.from_numpy(C.view(np.uint8).reshape(-1).copy()).to(dev)
            # resampleChroma works on frames: the chroma planes behind a Y plane of 2 h x 2 w samples that it neither reads nor writes
            at_in, at_out = pixfmt.planeOffsets(FMT[ds], 2 * w, 2 * h)[1], pixfmt.planeOffsets(FMT[dd], 2 * w * scale, 2 * h * scale)[1]
            raw = torch.zeros((pixfmt.frameBytes(FMT[ds], 2 * w, 2 * h),), dtype=torch.uint8, device=dev)
            raw[at_in:] = codes
            frame = torch.zeros((pixfmt.frameBytes(FMT[dd], 2 * w * scale, 2 * h * scale),), dtype=torch.uint8, device=dev)
            ip.resampleChroma(FMT[ds], FMT[dd], 2 * w, 2 * h, scale, method, loc)(raw, frame)
            fitted = torch.zeros((frame.numel() - at_out,), dtype=torch.uint8, device=dev)
            ip.fitPlanes(ds, dd, 2, h, w, h * scale, w * scale, method, loc)(codes, fitted)
            dt = np.uint8 if dd == 8 else np.dtype('<u2')
            a, b = frame[at_out:].cpu().numpy().view(dt), fitted.cpu().numpy().view(dt)
            bad = a != b
            if bad.any():
                i = int(np.argmax(bad))
                print('{} {} {}x{} x{} {}->{}: {} of {} samples differ, the first at {} (plane, row, column {}): resampleChroma {} fitPlanes {}'.format(
                    method, loc, h, w, scale, ds, dd, int(bad.sum()), bad.size, i, np.unravel_index(i, (2, h * scale, w * scale)), int(a[i]), int(b[i])))
            assert not bad.any(), (method, loc, h, w, scale, ds, dd)
            assert (a == pixfmt.resampleChroma(C, FMT[ds], FMT[dd], scale, method, loc).reshape(-1)).all(), (method, loc, h, w, scale, ds, dd)          # (and the definition's)
