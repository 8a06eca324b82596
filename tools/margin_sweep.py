#!/usr/bin/env python
"""How much of the 1e-3 budget the default arithmetic ('mixed': n split-operand blocks, fp8 corrections, fp8 low parts) keeps when the WEIGHTS change (the
defaults were tuned on a2's real weights, a4-synth and a few uint8-noise frames).  The engine's own exact mode ('fp16x3', pinned to the oracle at 2e-5) is the
transfer standard, as in tests/test_gpu_fullsize.py.  Variants: the 3x3 64->64 trunk weights (conv_input2, every ARSB) scaled by s -- activations and the
residual stream swing s^k times wider -- and an independent Gaussian perturbation of every conv weight by 10 % of its tensor's rms.
    python tools/margin_sweep.py [a4 a2]        -> worst tile (max-abs vs exact mode) per variant, uint8-noise and natural 256^2 tiles

SEDN keys (l25): the question is two-way -- does plain fp16 hold, or does the checkpoint run in 'fp16x3' -- so the sweep is fp16 against fp16x3 over EVERY 256-px
plane-tile of a 1080p uint8-noise frame (5 x 8 tiles, the last row / column anchored at the frame's edge as the planner does: 120 plane-tiles), beside the figure the
load-time measurement takes on its twelve-tile sample.  Their ratio is what kCalibInflateSEDN (csrc/calibrate.cpp) has to cover.  Variants: as shipped, and rblock.4
(the 64 -> 256 conv of every block) scaled by s -- the perturbed checkpoints of tests/test_gpu_sedn_calibrate.py.
    python tools/margin_sweep.py l25            -> per variant: sample, all-tile worst, ratio      (kept in profiles/margin_sweep_sedn.txt)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import golden_defs as gd  # noqa: E402
from moephoto_amd import models  # noqa: E402
from moephoto_amd.weights import load_state_dict_file  # noqa: E402


def variants(sd):
    trunk = [k for k in sd if k.startswith('conv_input2') or (k.startswith('convt_F') and k.endswith('weight') and sd[k].ndim == 4)]
    yield 'as shipped', dict(sd)
    for s in (0.85, 1.15, 1.3):
        v = dict(sd)
        for k in trunk:
            v[k] = (sd[k] * np.float32(s)).astype(np.float32)
        yield 'trunk weights x %.2f' % s, v
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        v = dict(sd)
        for k in sd:
            if sd[k].ndim == 4:
                v[k] = (sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.1 * np.sqrt(np.mean(sd[k] ** 2)))).astype(np.float32)
        yield 'every conv weight + N(0, (0.1 rms)^2), seed %d' % seed, v


SEDN_INFLATE = 1.30          # kCalibInflateSEDN of csrc/calibrate.cpp: calibrate() reports measured x this


def sedn_variants(sd):
    yield 'as shipped', dict(sd)
    for s in (1.25, 1.5, 2.0):
        yield 'rblock.4 x %.2f' % s, {k: ((v * np.float32(s)).astype(np.float32) if k.endswith('rblock.4.weight') else v) for k, v in sd.items()}


def frame_tiles(frame, crop=256):
    """every plane-tile of a (C, H, W) frame: crop-px tiles, the last row / column anchored at the edge -> (C * rows * cols, crop, crop)"""
    C, H, W = frame.shape
    tops = sorted(set(min(t, H - crop) for t in range(0, H, crop)))
    lefts = sorted(set(min(t, W - crop) for t in range(0, W, crop)))
    return np.stack([frame[c, t:t + crop, l:l + crop] for t in tops for l in lefts for c in range(C)])


def sweep_sedn(key):
    sd0 = gd.state_dict_for(key, load_state_dict_file)
    for name, sd in sedn_variants(sd0):
        ms = {}
        for prec in ('fp16', 'fp16x3'):
            ms[prec] = models.SEDN()
            ms[prec].precision = prec
            ms[prec].load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in sd.items()})
            ms[prec].eval().to(dtype=torch.float32, device='cuda:0')
        predicted = ms['fp16'].calibrate()[1]
        sample = predicted / SEDN_INFLATE
        line = '%-3s %-18s sample (12 tiles of 3 x 256 x 256) %.3e' % (key, name, sample)
        for seed in (0, 1):
            tiles = frame_tiles(gd.noise_u8(seed, (3, 1080, 1920)).astype(np.float32) / np.float32(255))
            per = []
            for c in range(0, len(tiles), 12):
                xd = torch.from_numpy(tiles[c:c + 12, None]).cuda()
                y = ms['fp16'](xd)[-1]
                want = ms['fp16x3'](xd)[-1]
                per += (y - want).abs().amax(dim=(1, 2, 3)).tolist()
            line += ' | 1080p frame %d: worst of %d plane-tiles %.3e = %.3f x sample (median %.3e, |y| <= %.2f)' % (seed, len(per), max(per), max(per) / sample, float(np.median(per)), float(want.abs().amax()))
        print(line, flush=True)


def main():
    keys = sys.argv[1:] or ['a4', 'a2']
    for key in keys:
        arch = gd.MODELS[key][0]
        if arch == 'sedn':
            sweep_sedn(key)
            continue
        sd0 = gd.state_dict_for(key, load_state_dict_file)
        ctor = {'net2x': models.Net2x, 'net3x': models.Net3x, 'net4x': models.Net4x, 'netdn': models.NetDN}[arch]
        for name, sd in variants(sd0):
            m = ctor()
            m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in sd.items()})
            m = m.eval().to(dtype=torch.float32, device='cuda:0')
            # what the load-time calibration settled on for THESE weights (round 6: twelve noise tiles of 3 x 256 x 256, measured x 1.10 = predicted full-frame worst tile):
            # the sweep below is the full-frame figure that prediction stands for
            cal = '{} / {} blocks'.format(m.resolved_precision(), m.exact_blocks())
            r = m.calibrate()
            if r is not None:
                infl = 1.30 if arch == 'netdn' else 1.10      # (kCalibInflateDN / kCalibInflate of csrc/calibrate.cpp)
                cal += ', calibrate() = ({}, predicted {:.3e} = measured {:.3e} x {:.2f})'.format(r[0], r[1], r[1] / infl, infl)
            worst = {}
            for kind in ('noise_u8', 'natural'):
                w = 0.0
                for seed in range(4):
                    x = (gd.noise_u8(seed, (12, 256, 256)).astype(np.float32) / np.float32(255)) if kind == 'noise_u8' else gd.natural_image(200 + seed, (12, 256, 256))
                    xd = torch.from_numpy(x[:, None]).cuda().half().float()
                    y = m.set_precision('auto')(xd)[-1]
                    want = m.set_precision('fp16x3')(xd)[-1]
                    w = max(w, float((y - want).abs().amax()))
                    rng_out = float(want.abs().amax())
                worst[kind] = (w, rng_out)
            print('%-3s %-52s noise_u8 %.3e (|y| <= %.2f)   natural %.3e | %s' % (key, name, worst['noise_u8'][0], worst['noise_u8'][1], worst['natural'][0], cal), flush=True)


if __name__ == '__main__':
    main()
