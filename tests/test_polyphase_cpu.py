"""The two integer polyphase definitions without a device (DESIGN.md sections 15 and 16): pixfmt.resampleChroma and pixfmt.fitPlanes share their arithmetic
(_polyAxis / _polyPlanes, _cubic, _quantRow), and what they compute is held here to bytes recorded BEFORE that arithmetic was shared, when each function still
carried its own copy: tests/golden/polyphase_digests.json holds the parameters, the seeds and one sha256 per (method, loc, depth pair) over the outputs of every
scale (resampleChroma) or target size (fitPlanes), in the file's order.  Nothing here may regenerate that file from the code under test.

Also here: at integer ratios the two definitions are one filter -- resampleChroma(C, .., s) == fitPlanes(C, .., h s, w s), byte for byte."""
import hashlib
import json
import os

import numpy as np
import pytest

from moephoto_amd import pixfmt

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'polyphase_digests.json')))
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
METHODS = ('nearest', 'bilinear', 'bicubic')
LOCS = ('center', 'left')


def codes(section, depth):
    """The section's input planes at `depth`: random codes below 2^depth from the seed the file stores, 0 and the all-ones code planted."""
    g = GOLDEN[section]
    c = np.random.default_rng(g['seeds'][str(depth)]).integers(0, 1 << depth, size=tuple(g['shape']))
    c.reshape(-1)[3] = 0
    c.reshape(-1)[-4] = (1 << depth) - 1
    return c.astype(np.uint8 if depth == 8 else '<u2')


def chroma_outputs(method, loc, ds, dd):
    x = codes('chroma', ds)
    return [pixfmt.resampleChroma(x, FMT[ds], FMT[dd], s, method, loc) for s in GOLDEN['chroma']['scales']]


def fit_outputs(method, loc, ds, dd):
    x = codes('fit', ds)
    return [pixfmt.fitPlanes(x, ds, dd, oh, ow, method, loc) for oh, ow in GOLDEN['fit']['sizes']]


def digest(outputs, dd, shapes):
    h = hashlib.sha256()
    for y, shape in zip(outputs, shapes):
        assert y.dtype == (np.uint8 if dd == 8 else np.dtype('<u2')) and y.shape == shape, (y.dtype, y.shape, shape)
        h.update(np.ascontiguousarray(y).tobytes())
    return h.hexdigest()


def test_the_file_holds_the_cases_the_definitions_are_held_to():
    c, f = GOLDEN['chroma'], GOLDEN['fit']
    assert c['shape'] == [2, 9, 17] and c['scales'] == [1, 2, 3, 4, 8, 16] and f['shape'] == [2, 13, 17]
    assert f['sizes'] == [[7, 9], [13, 17], [20, 26], [4, 5], [52, 68]]
    for g in (c, f):
        assert g['pairs'] == [[10, 8], [8, 16], [16, 10]]
        assert sorted(g['digests']) == sorted('{}/{}/{}-{}'.format(m, l, ds, dd) for m in METHODS for l in LOCS for ds, dd in g['pairs'])


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_resamplechroma_gives_the_recorded_bytes(method, loc):
    g = GOLDEN['chroma']
    _, h, w = g['shape']
    for ds, dd in g['pairs']:
        got = digest(chroma_outputs(method, loc, ds, dd), dd, [(2, h * s, w * s) for s in g['scales']])
        assert got == g['digests']['{}/{}/{}-{}'.format(method, loc, ds, dd)], (method, loc, ds, dd)


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_fitplanes_gives_the_recorded_bytes(method, loc):
    g = GOLDEN['fit']
    for ds, dd in g['pairs']:
        got = digest(fit_outputs(method, loc, ds, dd), dd, [(2, oh, ow) for oh, ow in g['sizes']])
        assert got == g['digests']['{}/{}/{}-{}'.format(method, loc, ds, dd)], (method, loc, ds, dd)


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_at_integer_ratios_the_two_definitions_are_one_filter(method, loc):
    g = GOLDEN['chroma']
    _, h, w = g['shape']
    for ds, dd in g['pairs']:
        x = codes('chroma', ds)
        for s, want in zip(g['scales'], chroma_outputs(method, loc, ds, dd)):
            got = pixfmt.fitPlanes(x, ds, dd, h * s, w * s, method, loc)
            bad = got != want
            assert got.dtype == want.dtype and not bad.any(), '{} {} x{} {}->{}: {} samples differ, the first at {}'.format(
                method, loc, s, ds, dd, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))
