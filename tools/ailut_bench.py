#!/usr/bin/env python
"""The AiLUT generator net (measurement tool; results: profiles/ailut/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/ailut_bench.py generator [--rounds 9] [--reps 50] [--out FILE.json]
    python tools/ailut_bench.py streams   [--models a4,a2] [--frames 24] [--warmup 4] [--rounds 9] [--out FILE.json]
    python tools/ailut_bench.py summary DIR          (DIR holds generator.json / streams.json / off.json / bench.json: whichever exist are written up as DIR/summary.md)

generator  one process, `rounds` alternating rounds of `reps` back-to-back runs between device events, microseconds per run, on a 1080p and an 8K bgr48le frame at
           d = 33, ranks = 3: A = moe_ailut_run (eight launches); B = the same functional graph in fp32 through torch eager on the same device and the same input
           (F.interpolate .. cumsum, the table re-laid as the handle keeps it).  Gate: A's median <= B's median.  Each of A's launches alone (moe_ailut_stage) in
           the same rounds.
streams    the 1080p bgr48le streams of a4 (-> 8K) and a2 (-> 4K), ring depth 2, with a fixed-table 'lut' step and with the generator's step, alternating `rounds`
           times in one process.  Gate: the compute stage's growth <= 2 x the generator's stand-alone time on a frame of the stream's output size.

The streams without either step against a checkout of the parent commit: tools/lut3d_bench.py off PARENT_TREE measures exactly that."""
import argparse
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
import chroma_bench as cb          # noqa: E402
import lut3d_bench as lb           # noqa: E402  (the frames, the device timer and the stream legs are that tool's)

median, H, W = cb.median, cb.H, cb.W
D, RANKS, GATE_STREAM = 33, 3, 2.0
STAGES = ('to_float_thumb_kernel', 'conv 1', 'conv 2', 'conv 3', 'conv 4', 'conv 5', 'heads', 'table')


def _state_dict():
    cb._path(HERE)
    import ailut_util as au
    return au.stateDict(2024, D, RANKS)


def _torch_graph(sd, dev):
    """f(frame) -> (entries (d^3, 4), vertices): torch eager in fp32 on the device, the parameters uploaded once."""
    import torch
    import torch.nn.functional as F
    from moephoto_amd import ailut
    p = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}

    def f(frame):          # frame: (H, W, 3) int16 storage of uint16 samples, bgr
        x = (frame.to(torch.int32) & 0xffff).to(torch.float32) * (1.0 / 65536.0)
        x = F.interpolate(x.flip(2).permute(2, 0, 1)[None], size=(256, 256), mode='bilinear', align_corners=False)
        for i in range(5):
            x = F.leaky_relu(F.conv2d(x, p['backbone.{}.0.weight'.format(i)], p['backbone.{}.0.bias'.format(i)], stride=2, padding=1), 0.2)
            if i < 4:
                x = F.instance_norm(x, weight=p['backbone.{}.2.weight'.format(i)], bias=p['backbone.{}.2.bias'.format(i)], eps=1e-5)
        feat = F.adaptive_avg_pool2d(x, 2).reshape(1, -1)
        w = F.linear(feat, p[ailut.KEY_H0 + '.weight'], p[ailut.KEY_H0 + '.bias'])
        table = F.linear(w, p[ailut.KEY_BANK + '.weight']).reshape(3, D ** 3)
        entries = torch.cat([table.t(), torch.zeros((D ** 3, 1), device=dev)], 1).contiguous()
        v = F.pad(F.linear(feat, p[ailut.KEY_G + '.weight'], p[ailut.KEY_G + '.bias']).reshape(1, 3, D - 1).softmax(-1).cumsum(-1), (1, 0))
        return entries, v
    return f


def generator(args):
    cb._path(HERE)
    import torch
    from moephoto_amd import _lib, ailut, lut3d
    from moephoto_amd.imageProcess import _AilutHandle, _LutHandle
    _lib.require_device()
    torch.backends.cudnn.benchmark = True          # (torch's leg picks its fastest conv kernels in the warm-up runs)
    sd = _state_dict()
    L, dev = _lib.lib(), torch.device('cuda:0')
    gen, lut, eager = _AilutHandle(ailut.loadParams(sd), 0), _LutHandle(lut3d.identity(D), lut3d.uniform(D), 0), _torch_graph(sd, dev)
    result = {'d': D, 'ranks': RANKS, 'rounds': args.rounds, 'reps': args.reps, 'frames': {}}
    for name, (h, w) in (('1080p', (1080, 1920)), ('8K', (4320, 7680))):
        src = lb._frame16('smooth', h, w, dev)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        legs = {'hip': lambda: _lib.check(L.moe_ailut_run(gen._h, src.data_ptr(), 16, h, w, 0, lut._h, stream())), 'torch': lambda: eager(src)}
        for k, stage in enumerate(STAGES):
            legs[stage] = (lambda k: lambda: _lib.check(L.moe_ailut_stage(gen._h, k, src.data_ptr(), 16, h, w, 0, lut._h, stream())))(k)
        us = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, f in legs.items():
                us[leg].append(lb._device_us(f, args.reps))
        r = {leg: {'us': v, 'median': median(v), 'spread': round(max(v) - min(v), 2)} for leg, v in us.items()}
        r['stages_sum'] = round(sum(r[s]['median'] for s in STAGES), 2)
        r['gate'] = {'hip_us': r['hip']['median'], 'torch_us': r['torch']['median'], 'holds': bool(r['hip']['median'] <= r['torch']['median'])}
        result['frames'][name] = r
        print('{}: hip {} us, torch {} us'.format(name, r['hip']['median'], r['torch']['median']), file=sys.stderr, flush=True)
    cb._emit(result, args.out)


def _steps(key, form):
    steps = lb._steps(key, form == 'lut')
    if form == 'ailut':
        steps.append({'op': 'dehaze', 'model': 'AiLUT_sRGB_3'})
    return steps


def streams(args):
    tmp = cb._setup(HERE)
    import torch
    from moephoto_amd import _lib, ailut, lut3d, procedure, weights
    from moephoto_amd.imageProcess import _AilutHandle, _LutHandle
    from moephoto_amd.config import config
    sd = _state_dict()
    root = os.path.join(tmp, 'zoo')          # a modelRoot of its own: the tests' zoo linked in, the generator's checkpoint beside it at the reference's path
    os.makedirs(os.path.join(root, 'model'))
    for name in os.listdir(os.path.join(config.modelRoot, 'model')):
        os.symlink(os.path.join(config.modelRoot, 'model', name), os.path.join(root, 'model', name))
    path = os.path.join(root, ailut.MODELS['AiLUT_sRGB_3'])
    os.makedirs(os.path.dirname(path))
    weights.save_state_dict_file(sd, path)
    config.modelRoot = root
    frames = lb._noise_frames(args.warmup + args.frames)
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'models': {}}
    L, dev = _lib.lib(), torch.device('cuda:0')
    gen, lut = _AilutHandle(ailut.loadParams(sd), 0), _LutHandle(lut3d.identity(D), lut3d.uniform(D), 0)
    for key in args.models.split(','):
        res = {name: {'fps': [], 'stage_ms_per_frame': []} for name in ('lut', 'ailut')}
        for _ in range(args.rounds):
            for name in res:
                stream = procedure.genFrameStream(_steps(key, name), W, H, cb.DEPTH, timing=True)
                fps, stages = cb._leg(stream, frames, args.warmup)
                res[name]['edge'] = stream.edge
                stream.close()
                res[name]['fps'].append(fps)
                res[name]['stage_ms_per_frame'].append(stages)
                print('{} {}: {} fps, compute {} ms'.format(key, name, fps, stages['compute_ms']), file=sys.stderr, flush=True)
        for r in res.values():
            r['fps_median'] = median(r['fps'])
            r['compute_ms_median'] = median([s['compute_ms'] for s in r['stage_ms_per_frame']])
            r['compute_ms_spread'] = round(max(s['compute_ms'] for s in r['stage_ms_per_frame']) - min(s['compute_ms'] for s in r['stage_ms_per_frame']), 3)
        s = int(key[-1])
        oh, ow = s * H, s * W
        src = lb._frame16('smooth', oh, ow, dev)
        f = lambda: _lib.check(L.moe_ailut_run(gen._h, src.data_ptr(), 16, oh, ow, 0, lut._h, torch.cuda.current_stream().cuda_stream))
        own = median([lb._device_us(f, 20) for _ in range(5)])
        inc = round(res['ailut']['compute_ms_median'] - res['lut']['compute_ms_median'], 3)
        res['gate'] = {'generator_us': own, 'compute_increase_ms': inc, 'bar_ms': round(GATE_STREAM * own / 1e3, 3), 'holds': bool(inc <= GATE_STREAM * own / 1e3)}
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    cb._emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.dir)
    load = lambda n: json.load(open(os.path.join(d, n))) if os.path.exists(os.path.join(d, n)) else None
    g, s = load('generator.json'), load('streams.json')
    out = ['# The AiLUT generator net: measurements (tools/ailut_bench.py; one MI355X)', '']
    if g:
        out += ['## Generator gate: moe_ailut_run against the same graph in fp32 through torch eager, d = {}, ranks = {}, {} alternating rounds of {} runs'.format(
            g['d'], g['ranks'], g['rounds'], g['reps']), '', '| frame | leg | median us | spread us |', '|---|---|---|---|']
        for name, r in g['frames'].items():
            for leg in ('hip', 'torch') + STAGES:
                out.append('| {} | {} | {} | {} |'.format(name, leg, r[leg]['median'], r[leg]['spread']))
            out.append('| {} | the eight launches alone, summed | {} | |'.format(name, r['stages_sum']))
            out.append('| {} | **gate (hip <= torch): {}** | | |'.format(name, 'held' if r['gate']['holds'] else 'MISSED'))
        out.append('')
    if s:
        out += ['## Stream gate: the compute stage with the generator\'s step against a fixed-table lut step, {} rounds of {} frames, ring depth {}'.format(
            s['rounds'], s['frames'], s['depth']), '', '| stream | form | edge | fps | compute ms / frame | spread |', '|---|---|---|---|---|---|']
        for key, r in s['models'].items():
            for form in ('lut', 'ailut'):
                out.append('| {} | {} | {} | {} | {} | {} |'.format(key, form, r[form]['edge'], r[form]['fps_median'], r[form]['compute_ms_median'], r[form]['compute_ms_spread']))
            gt = r['gate']
            out.append('| {} | **gate: +{} ms against a bar of {} ms (twice the generator\'s {} us): {}** | | | | |'.format(
                key, gt['compute_increase_ms'], gt['bar_ms'], gt['generator_us'], 'held' if gt['holds'] else 'MISSED'))
        out.append('')
    o, b = load('off.json'), load('bench.json')
    if o:
        out += ['## No cost when off: the streams without the step, this tree against a checkout of the parent commit (tools/lut3d_bench.py off), alternating child processes, {} rounds of {} frames'.format(
            o['rounds'], o['frames']), '', '| stream | parent fps (median; all) | tree fps (median; all) | parent compute ms | tree compute ms | parent\'s own spread (fps) | within it |', '|---|---|---|---|---|---|---|']
        for key, m in o['models'].items():
            out.append('| {} | {}; {} | {}; {} | {} | {} | {} | {} |'.format(key, m['parent']['fps_median'], m['parent']['fps'], m['tree']['fps_median'], m['tree']['fps'], m['parent']['compute_ms_median'],
                                                                    m['tree']['compute_ms_median'], m['parent_spread']['fps'], 'yes' if m['holds'] else 'NO'))
        out += ['', 'The parent checkout ran with this tree\'s library (a superset of its exports; the kernels it runs are compiled from unchanged sources): what the two legs', 'compare is the Python above it, which is where this change touches chains without the step.', '']
    if b:
        out += ['## bench.py', '', '`bench.py --gpus 1 --steps {} --warmup {}` (the a4 frame path, untouched): {} MP/s in {} run, beside the documented {} - {} MP/s.'.format(
            b['steps'], b['warmup'], b['value'], b['runs'], *b['documented_range']), '']
    out += ['## Not measured', '', 'What bounds each launch (no counter run; every launch is a few microseconds of work behind a launch: latency-bound by its size). Planar sources, `reuse=True`,',
            '`views=True`, 8-bit sources and strengths other than 1 in the streams. Real video and real checkpoints: the weights are seeded, no checkpoint of this net ships with the project.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(out))
    print(os.path.join(d, 'summary.md'))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('generator', 'streams', 'summary'))
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--models', default='a4,a2')
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--out')
    a = ap.parse_args()
    {'generator': generator, 'streams': streams, 'summary': summary}[a.mode](a)
