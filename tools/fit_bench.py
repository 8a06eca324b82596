#!/usr/bin/env python
"""Fitted sizes on 4:2:0 planes (measurement tool; results: profiles/fit/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/fit_bench.py kernel  [--rounds 7] [--reps 30] [--out FILE.json]
    python tools/fit_bench.py streams [--models a4,a2] [--frames 16] [--warmup 4] [--rounds 3] [--out FILE.json]
    python tools/fit_bench.py summary DIR          (DIR holds kernel.json / streams.json / off.json: whichever exist are written up as DIR/summary.md)

kernel   one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/chroma_bench.py):
         A = resize_kernel_fit on one 7680 x 4320 plane of 16-bit codes -> 3840 x 2160 at depth 10, bicubic;
         B = what the float route spends on the same plane: moe_resize (bicubic, fp16, 7680 x 4320 -> 3840 x 2160) followed by moe_to_output (depth 10).
         Gate: A's median <= B's median - B's own round-to-round spread.  Also timed, without a gate: the fit of a 3840 x 2160 plane at 3/2 up and at 3/4 down, the
         chroma pair of the gate's frame (2 x 3840 x 2160 -> 2 x 1920 x 1080) and the 4 : 1 limit (7680 x 4320 -> 1920 x 1080).
streams  planar streams with a size on the output step beside the only way to that size without it, the bgr48le chain ending in a resize step, alternating `rounds`
         times in one process: a4, 1080p -> 4K (fitted from 8K) and a2, 720p -> 1080p, each with chroma 'net' and 'bicubic'; frames per second and the ring's
         compute-stage ms per frame.
The planar streams WITHOUT the new keys against a checkout of the parent commit: `tools/chroma_bench.py off PARENT_TREE --out DIR/off.json` measures exactly those
streams as alternating child processes; `summary` writes its result up here.

a4 uses the synthetic weights of tests/golden_defs.py (as bench.py does); every kernel's time is independent of the data."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP, DEPTH = 256, 2


def median(v):
    return sorted(v)[len(v) // 2]


def _emit(result, out):
    print(json.dumps(result), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(result, open(out, 'w'), indent=1)


def _path(root):
    for p in (root, os.path.join(root, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)


def kernel(args):
    _path(HERE)
    import torch
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import fitPlanes
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    codes = lambda C, h, w: torch.randint(0, 65536, (C * h * w,), dtype=torch.int32, device=dev).to(torch.int16).view(torch.uint8)

    def fit(C, h, w, oh, ow):
        src, out, f = codes(C, h, w), torch.empty((C * oh * ow * 2,), dtype=torch.uint8, device=dev), fitPlanes(16, 10, C, h, w, oh, ow, 'bicubic')
        f(src, out)
        return (lambda: f(src, out)), C * (h * w + oh * ow) * 2, f.info(dev)
    H8, W8, H4, W4 = 4320, 7680, 2160, 3840
    x = torch.rand((1, H8, W8), dtype=torch.float16, device=dev)
    y = torch.empty((1, H4, W4), dtype=torch.float16, device=dev)
    q = torch.empty((H4 * W4,), dtype=torch.int16, device=dev)

    def floats():
        _lib.check(L.moe_resize(x.data_ptr(), y.data_ptr(), _lib.F16, 1, H8, W8, H4, W4, _lib.RESIZE_MODES['bicubic'], 0, st))
        _lib.check(L.moe_to_output(y.data_ptr(), _lib.F16, H4, W4, 1, 10, q.data_ptr(), _lib.U16, 0, st))
    cases, moved, tiles = {}, {}, {}
    for name, geo in (('A_fit_8K_to_4K', (1, H8, W8, H4, W4)), ('fit_4K_up_3_2', (1, H4, W4, H4 * 3 // 2, W4 * 3 // 2)), ('fit_4K_down_3_4', (1, H4, W4, H4 * 3 // 4, W4 * 3 // 4)),
                      ('fit_chroma_pair_4K_to_1080p', (2, H4, W4, H4 // 2, W4 // 2)), ('fit_8K_to_1080p_4_to_1', (1, H8, W8, H4 // 2, W4 // 2))):
        cases[name], moved[name], tiles[name] = fit(*geo)
    cases['B_moe_resize_then_moe_to_output'], moved['B_moe_resize_then_moe_to_output'] = floats, (H8 * W8 + 3 * H4 * W4) * 2

    def device_us(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            f()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / args.reps, 2)
    rounds = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, f in cases.items():
            rounds[k].append(device_us(f))
    res = {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2), 'bytes': moved[k],
               'GB_per_s': round(moved[k] / median(v) / 1e3, 1)} for k, v in rounds.items()}
    for k, t in tiles.items():
        res[k]['tile'], res[k]['lds_bytes'] = list(t['tile']), t['lds']
    a, b = res['A_fit_8K_to_4K'], res['B_moe_resize_then_moe_to_output']
    a['bar_us'] = round(b['median_us'] - b['spread_us'], 2)
    a['holds'] = a['median_us'] <= a['bar_us']
    _emit({'reps': args.reps, 'rounds': args.rounds, 'timing': 'device events around `reps` back-to-back launches', 'cases': res}, args.out)


def _setup():
    _path(HERE)
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_fit_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    return tmp


def _leg(stream, frames, warmup):
    """warmup untimed frames, then the rest between two host clock reads, the second behind a device synchronise -> (fps, the ring's compute ms per frame)"""
    import torch
    from moephoto_amd import procedure

    def run(data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(stream, io.BytesIO(data).read, lambda buf: None)
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0
    run(b''.join(frames[:warmup]), warmup)
    st = stream.backend.stats
    for k in st:
        st[k] = 0
    n = len(frames) - warmup
    dt = run(b''.join(frames[warmup:]), n)
    return round(n / dt, 3), round(st['compute_ms'] / max(1, st['frames']), 3)


def streams(args):
    tmp = _setup()
    import numpy as np
    from moephoto_amd import pixfmt, procedure
    rng = np.random.default_rng(2024)
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'streams': {}}
    for key, (w, h), (W, H) in (('a4', (1920, 1080), (3840, 2160)), ('a2', (1280, 720), (1920, 1080))):
        if key not in args.models.split(','):
            continue
        sr = {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}
        n = args.frames + args.warmup
        planar = [rng.integers(0, 1 << 10, pixfmt.frameBytes('yuv420p10le', w, h) // 2, dtype=np.uint16).tobytes() for _ in range(n)]
        rgb = [rng.integers(0, 65536, w * h * 3, dtype=np.uint16).tobytes() for _ in range(n)]
        size = {'op': 'output', 'width': W, 'height': H, 'fit': 'bicubic'}
        configs = {'planes_net_fit': ([{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, dict(sr), dict(size)], planar),
                   'planes_bicubic_fit': ([{'op': 'buffer', 'pixFmt': 'yuv420p10le', 'chroma': 'bicubic'}, dict(sr), dict(size)], planar),
                   'bgr48le_resize': ([{'op': 'buffer', 'bitDepth': 16}, dict(sr), {'op': 'resize', 'width': W, 'height': H, 'method': 'bicubic'}], rgb)}
        res = {name: {'fps': [], 'compute_ms': []} for name in configs}
        for _ in range(args.rounds):
            for name, (steps, frames) in configs.items():
                stream = procedure.genFrameStream([dict(s) for s in steps], w, h, DEPTH, timing=True)
                fps, comp = _leg(stream, frames, args.warmup)
                res[name]['edge'] = stream.edge
                stream.close()
                res[name]['fps'].append(fps)
                res[name]['compute_ms'].append(comp)
        for r in res.values():
            r['fps_median'], r['compute_ms_median'] = median(r['fps']), median(r['compute_ms'])
        result['streams']['{} {}x{} -> {}x{}'.format(key, w, h, W, H)] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.dir)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, s, o = load('kernel.json'), load('streams.json'), load('off.json')
    lines = ['# Fitted sizes on 4:2:0 planes: measurements (`tools/fit_bench.py`)', '',
             'MI355X, one device.  Everything below is written by `fit_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '']
    lines += ['## Kernel gate: `resize_kernel_fit` against the float route\'s two passes', '']
    if k:
        lines += ['One plane of 7680 x 4320 16-bit codes -> 3840 x 2160 at depth 10, bicubic; ' + k['timing'] + ', {} rounds of {} launches, the legs alternating in one process.'.format(
            k['rounds'], k['reps']), '', '| leg | median µs | fastest | spread over rounds | bytes moved | GB/s | tile | LDS bytes |', '|---|---|---|---|---|---|---|---|']
        for name, r in k['cases'].items():
            lines.append('| `{}` | {} | {} | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['bytes'], r['GB_per_s'],
                                                                        'x'.join(map(str, r['tile'])) if 'tile' in r else '', r.get('lds_bytes', '')))
        a = k['cases']['A_fit_8K_to_4K']
        lines += ['', 'Gate (A <= B - B\'s spread = {} µs): **{}**.'.format(a['bar_us'], 'holds' if a['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: a size on the output step beside the bgr48le chain that ends in a resize step', '']
    if s:
        lines += ['Ring depth {}, distinct noise frames, {} timed frames per leg after {} warm-up frames, the configurations alternating {} times in one process.'.format(
            s['depth'], s['frames'], s['warmup'], s['rounds']), '', '| stream | configuration | edge | fps (legs) | fps median | compute ms (legs) | median |', '|---|---|---|---|---|---|---|']
        for key, m in s['streams'].items():
            for name, r in m.items():
                lines.append('| {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r.get('edge', ''), r['fps'], r['fps_median'], r['compute_ms'], r['compute_ms_median']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## No cost when off: the planar streams with no new key, against the parent commit (`tools/chroma_bench.py off`)', '']
    if o:
        lines += ['Alternating child processes ({}), {} timed frames per leg after {} warm-up frames.'.format(', '.join(o['order']), o['frames'], o['warmup']), '',
                  '| stream | parent fps (legs) | median | tree fps (legs) | median | parent\'s spread | tree - parent | within |', '|---|---|---|---|---|---|---|---|']
        for key, m in o['models'].items():
            lines.append('| {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, m['parent']['fps'], m['parent']['fps_median'], m['tree']['fps'], m['tree']['fps_median'],
                                                                         m['parent_spread']['fps'], m['tree_against_parent']['fps'], 'yes' if m['holds'] else 'NO'))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'streams', 'summary'])
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--models', default='a4,a2')
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.mode == 'summary' and not args.dir:
        ap.error('summary needs a directory')
    if args.rounds is None:
        args.rounds = 7 if args.mode == 'kernel' else 3
    {'kernel': kernel, 'streams': streams, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
