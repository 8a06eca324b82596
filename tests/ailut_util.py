"""What the AiLUT generator's tests share: seeded checkpoints with the reference's key names (no checkpoint of this net is committed: nothing here comes from the
reference), the torch functional graph the definition and the device are held to, and test frames."""
import os
from collections import OrderedDict

import numpy as np

from moephoto_amd import ailut, weights

_made = {}


def stateDict(seed, d=33, ranks=3):
    """A state dict of float32 arrays: conv weights with fan-in scaling (activations stay O(1) through five blocks), gamma near 1, beta near 0; the bank's first
    column is the identity table and the first rank's bias 1, so that a table is the identity plus an image-dependent part."""
    key = (seed, d, ranks)
    if key not in _made:
        rng = np.random.default_rng(seed)
        sd = OrderedDict()
        for name, shape in ailut.paramShapes(d, ranks).items():
            if name.startswith('backbone') and name.endswith('.0.weight'):
                a = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * 9))
            elif name.startswith('backbone') and name.endswith('.2.weight'):
                a = 1.0 + 0.2 * (rng.random(shape) - 0.5)
            elif name.endswith('bias'):
                a = 0.2 * (rng.random(shape) - 0.5)
            elif name == ailut.KEY_BANK + '.weight':
                a = 0.3 * rng.standard_normal(shape)
                g = np.arange(d) / (d - 1.0)
                a[:, 0] = np.stack(np.broadcast_arrays(g[None, None, :], g[None, :, None], g[:, None, None])).reshape(-1)
            else:          # the two linear heads
                a = rng.standard_normal(shape) * (2.0 / np.sqrt(ailut.FEATURES))
            sd[name] = a.astype(np.float32)
        sd[ailut.KEY_H0 + '.bias'][0] = 1.0
        _made[key] = sd
    return _made[key]


def writeCheckpoint(root, model, sd):
    """The state dict as the zoo's legacy-format file at the reference's path under `root`."""
    path = os.path.join(str(root), ailut.MODELS[model])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    weights.save_state_dict_file(sd, path)
    return path


def torchForward(samples, srcBits, order, sd, dtype):
    """(thumbnail, table, vertices) as numpy float64 of the reference's graph in torch's functional ops at `dtype`, on the CPU: F.interpolate .. cumsum."""
    import torch
    import torch.nn.functional as F
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(dtype)
    x = torch.from_numpy(np.ascontiguousarray(samples).astype(np.float64)).to(dtype) / (65536.0 if srcBits == 16 else 255.0)
    if order == 'bgr':
        x = x.flip(2)
    thumb = F.interpolate(x.permute(2, 0, 1)[None], size=(ailut.SIZE, ailut.SIZE), mode='bilinear', align_corners=False)
    table, vertices = torchGenerate(thumb, sd, dtype)
    return thumb[0].double().numpy(), table, vertices


def torchGenerate(thumb, sd, dtype):
    import torch
    import torch.nn.functional as F
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(dtype)
    x = thumb if isinstance(thumb, torch.Tensor) else torch.from_numpy(np.asarray(thumb)).to(dtype)[None]
    for i in range(5):
        x = F.leaky_relu(F.conv2d(x, t('backbone.{}.0.weight'.format(i)), t('backbone.{}.0.bias'.format(i)), stride=2, padding=1), 0.2)
        if i < 4:
            x = F.instance_norm(x, weight=t('backbone.{}.2.weight'.format(i)), bias=t('backbone.{}.2.bias'.format(i)), eps=1e-5)
    f = F.adaptive_avg_pool2d(x, 2).reshape(1, -1)
    d = sd[ailut.KEY_G + '.weight'].shape[0] // 3 + 1
    w = F.linear(f, t(ailut.KEY_H0 + '.weight'), t(ailut.KEY_H0 + '.bias'))
    table = F.linear(w, t(ailut.KEY_BANK + '.weight')).reshape(3, d, d, d)
    intervals = F.linear(f, t(ailut.KEY_G + '.weight'), t(ailut.KEY_G + '.bias')).reshape(1, 3, d - 1).softmax(-1)
    vertices = F.pad(intervals.cumsum(-1), (1, 0), 'constant', 0)[0]
    return table.double().numpy(), vertices.double().numpy()


def frame(kind, w, h, bits, seed=0):
    """(h, w, 3) codes: 'noise', 'flat' (one colour: zero variance in every normalised layer but for the zero padding's border) or 'ramp' (smooth)."""
    top = (1 << bits) - 1
    if kind == 'noise':
        a = np.random.default_rng(seed).integers(0, top + 1, (h, w, 3))
    elif kind == 'flat':
        a = np.broadcast_to(np.array([0, 0, 0]) if seed % 2 else np.array([top * 2 // 5, top // 3, top * 3 // 4]), (h, w, 3))
    else:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([x * top // max(w - 1, 1), y * top // max(h - 1, 1), (x + y) * top // max(w + h - 2, 1)], -1)
    return np.ascontiguousarray(a).astype(np.uint8 if bits == 8 else np.uint16)
