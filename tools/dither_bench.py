#!/usr/bin/env python
"""Rounding and ordered dither in the quantising edges (measurement tool; results: profiles/dither/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/dither_bench.py kernel  [--rounds 7] [--reps 30] [--out FILE.json]
    python tools/dither_bench.py streams [--models a4,a2] [--frames 16] [--warmup 4] [--rounds 2] [--out FILE.json]
    python tools/dither_bench.py ramp    [--out FILE.json]
    python tools/dither_bench.py summary DIR          (DIR holds kernel.json / streams.json / ramp.json: whichever exist are written up as DIR/summary.md)

kernel   the a4 1080p -> 8K pool, one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch: each 8-bit edge
         plain and with 'ordered' on the same pool -- stitch_out_kernel<u8, 3, 4> / stitch_out_dither_kernel (unit scale), stitch_yuv_kernel<u8> / its twin,
         stitch_planes_kernel<u8> / its twin on the Y' plane.  Gate: the dithered leg's median <= the plain leg's median + the plain leg's own round-to-round spread.
streams  1080p frames through genFrameStream (ring depth 2, views=True, distinct noise frames), a4 -> 8K and a2 -> 4K, three legs alternating: bgr24 plain, bgr24 with
         {'op': 'output', 'dither': 'ordered'}, and bgr48le plain -- what has to be downloaded today to dither elsewhere -- with the bytes per finished frame beside it.
ramp     informational: an 8-bit horizontal-then-raster gradient frame (codes 51 .. 77 of 255, the CPU test's 0.2 .. 0.3) through a2, fp16; per mode the worst 8 x 8
         block-mean error of the delivered codes against the chain's own float result times 255, and the mean error.

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
H, W, CROP, DEPTH = 1080, 1920, 256, 2
for _p in (HERE, os.path.join(HERE, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def median(v):
    return sorted(v)[len(v) // 2]


def _emit(result, out):
    print(json.dumps(result), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(result, open(out, 'w'), indent=1)


def _device_us(f, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def _alternate(cases, rounds, reps):
    got = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            got[k].append(_device_us(f, reps))
    return {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2)} for k, v in got.items()}


def kernel(args):
    import torch
    from moephoto_amd import _lib, pixfmt, quant
    from moephoto_amd.imageProcess import TilePlan
    _lib.require_device()
    L, dev, st = _lib.lib(), torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream
    p1, p3 = TilePlan((1, H, W), 1 << 40, 1e-3, 5, 4, 8, CROP), TilePlan((3, H, W), 1 << 40, 1e-3, 5, 4, 8, CROP)
    pool1, pool3 = torch.rand(p1.pool_elems(1), device=dev), torch.rand(p3.pool_elems(3), device=dev)
    px = 16 * H * W
    out = torch.empty((px * 3,), dtype=torch.uint8, device=dev)
    rgb, yuv, pln = quant.flags('ordered', 8, 'rgb'), quant.flags('ordered', 8, 'yuv'), quant.flags('ordered', 8, 'planes')
    F16, U8 = _lib.F16, _lib.U8
    cases = {'stitch_out_kernel<u8, 3, 4>': lambda: _lib.check(L.moe_stitch_out(p3._h, 0, pool3.data_ptr(), None, 3, F16, 8, out.data_ptr(), U8, st)),
             'stitch_out ordered': lambda: _lib.check(L.moe_stitch_out(p3._h, 0, pool3.data_ptr(), None, 3, F16, 8 | rgb, out.data_ptr(), U8, st)),
             'stitch_yuv_kernel<u8, 4>': lambda: _lib.check(L.moe_stitch_yuv(p3._h, 0, pool3.data_ptr(), None, F16, 8, 0, 0, out.data_ptr(), st)),
             'stitch_yuv ordered': lambda: _lib.check(L.moe_stitch_yuv(p3._h, 0, pool3.data_ptr(), None, F16, 8 | yuv, 0, 0, out.data_ptr(), st)),
             'stitch_planes_kernel<u8, 4>': lambda: _lib.check(L.moe_stitch_planes(p1._h, 0, pool1.data_ptr(), None, 1, F16, 8, out.data_ptr(), st)),
             'stitch_planes ordered': lambda: _lib.check(L.moe_stitch_planes(p1._h, 0, pool1.data_ptr(), None, 1, F16, 8 | pln, out.data_ptr(), st))}
    res = _alternate(cases, args.rounds, args.reps)
    moved = {'stitch_out': px * (12 + 3), 'stitch_yuv': px * 12 + pixfmt.frameBytes('yuv420p', 4 * W, 4 * H), 'stitch_planes': px * (4 + 1)}
    gates = {}
    for k, r in res.items():
        r['bytes'] = moved[k.split('_kernel')[0].split(' ')[0]]
        r['GB_per_s'] = round(r['bytes'] / r['median_us'] / 1e3, 1)
    for plain, dith in (('stitch_out_kernel<u8, 3, 4>', 'stitch_out ordered'), ('stitch_yuv_kernel<u8, 4>', 'stitch_yuv ordered'), ('stitch_planes_kernel<u8, 4>', 'stitch_planes ordered')):
        a, b = res[dith], res[plain]
        a['bar_us'] = round(b['median_us'] + b['spread_us'], 2)
        a['holds'] = a['median_us'] <= a['bar_us']
        gates[dith] = a['holds']
    _emit({'geometry': 'a4 1080p -> 8K: (3 | 1, 1080, 1920) x4, tiles of 256, fp16 canvas rounding, 8-bit samples', 'reps': args.reps, 'rounds': args.rounds,
           'timing': 'device events around `reps` back-to-back launches', 'cases': res, 'gates': gates}, args.out)


def _setup():
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_dither_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    return tmp


def _leg(stream, frames, warmup):
    import torch
    from moephoto_amd import procedure
    sink = {'bytes': 0, 'frames': 0}

    def write(buf):
        sink['bytes'] += len(buf)
        sink['frames'] += 1

    def run(data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(stream, io.BytesIO(data).read, write)
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0
    if warmup:
        run(b''.join(frames[:warmup]), warmup)
    st = stream.backend.stats
    for k in st:
        st[k] = 0
    sink['bytes'] = sink['frames'] = 0
    n = len(frames) - warmup
    dt = run(b''.join(frames[warmup:]), n)
    return round(n / dt, 3), {k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'}, sink['bytes'] // max(1, sink['frames'])


def streams(args):
    tmp = _setup()
    import numpy as np
    from moephoto_amd import procedure
    rng = np.random.default_rng(2024)
    n = args.warmup + args.frames
    frames = {8: [rng.integers(0, 256, H * W * 3, dtype=np.uint8).tobytes() for _ in range(n)], 16: [rng.integers(0, 65536, H * W * 3, dtype=np.uint16).tobytes() for _ in range(n)]}
    legs = {'bgr24 plain': (8, None), 'bgr24 ordered': (8, 'ordered'), 'bgr48le plain': (16, None)}
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'source': '1080p, views=True', 'models': {}}
    for key in args.models.split(','):
        res = {name: {'fps': [], 'stage_ms_per_frame': []} for name in legs}
        for _ in range(args.rounds):
            for name, (bits, dither) in legs.items():
                steps = [{'op': 'buffer', 'bitDepth': bits}, {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}] + ([{'op': 'output', 'dither': dither}] if dither else [])
                stream = procedure.genFrameStream(steps, W, H, DEPTH, timing=True, views=True)
                fps, stages, nbytes = _leg(stream, frames[bits], args.warmup)
                stream.close()
                res[name]['fps'].append(fps)
                res[name]['stage_ms_per_frame'].append(stages)
                res[name]['bytes_per_frame'] = nbytes
        for r in res.values():
            r['fps_median'], r['fps_spread'] = median(r['fps']), round(max(r['fps']) - min(r['fps']), 3)
            for k in ('compute_ms', 'tobytes_ms', 'd2h_ms', 'h2d_ms', 'memcpy_ms'):
                r[k + '_median'] = median([s[k] for s in r['stage_ms_per_frame']])
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def ramp(args):
    tmp = _setup()
    import numpy as np
    from moephoto_amd import imageProcess as ip, procedure, runSR
    # 0.2 .. 0.3 in 8-bit codes of / 255, over the frame in raster order, as the CPU test's ramp: each row is nearly flat, rows rise slowly
    h, w = 128, 128
    codes = np.clip(np.rint(np.linspace(0.2, 0.3, h * w) * 255), 0, 255).astype(np.uint8).reshape(h, w)
    im = np.repeat(codes[:, :, None], 3, 2)
    opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0})
    y = ip.doCrop(opt, ip.toTorch(8)(im)).float().cpu().numpy().transpose(1, 2, 0).astype(np.float64) * 255
    result = {'frame': '{} x {} x 3, 8-bit codes of a 0.2 .. 0.3 raster ramp, a2, fp16'.format(h, w), 'modes': {}}
    for mode in ('none', 'round', 'ordered'):
        process, _ = procedure.genProcess([{'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}, {'op': 'output', 'dither': mode}])
        err = process(im).astype(np.float64) - y
        blocks = err.reshape(2 * h // 8, 8, 2 * w // 8, 8, 3).mean((1, 3))
        result['modes'][mode] = {'worst_block_mean_codes': float(np.abs(blocks).max()), 'mean_codes': float(err.mean())}
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.dir)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, s, r = load('kernel.json'), load('streams.json'), load('ramp.json')
    lines = ['# Rounding and ordered dither in the quantising edges: measurements (`tools/dither_bench.py`)', '',
             'MI355X, one device.  Everything below is written by `dither_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '']
    lines += ['## The 8-bit edges alone, on the a4 1080p -> 8K pool', '']
    if k:
        lines += [k['geometry'] + '; ' + k['timing'] + ', {} rounds of {} launches, the legs alternating in one process.'.format(k['rounds'], k['reps']), '',
                  '| leg | median µs | fastest | spread over rounds | rounds | bytes moved | GB/s | bar (plain median + its spread) | |', '|---|---|---|---|---|---|---|---|---|']
        for name, c in k['cases'].items():
            lines.append('| `{}` | {} | {} | {} | {} | {} | {} | {} | {} |'.format(name, c['median_us'], c['fastest_us'], c['spread_us'], c['rounds_us'], c['bytes'], c['GB_per_s'], c.get('bar_us', ''),
                                                                              '' if 'holds' not in c else ('**holds**' if c['holds'] else '**MISSED**')))
        lines += ['', 'Registers of the twins: `profiles/stitch/resources.md`.', '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: 1080p frames, ring depth 2, views', '']
    if s:
        lines += ['{} timed frames per leg after {} warm-up frames, the legs alternating {} times; stage times in ms per frame.'.format(s['frames'], s['warmup'], s['rounds']), '',
                  '| stream | leg | bytes per finished frame | fps (legs) | fps median | compute | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|']
        for key, m in s['models'].items():
            for name, c in m.items():
                lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, c['bytes_per_frame'], c['fps'], c['fps_median'], c['compute_ms_median'], c['d2h_ms_median'],
                                                                                  c['h2d_ms_median'], c['memcpy_ms_median']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## The ramp through a2 (informational)', '']
    if r:
        lines += [r['frame'] + '; the delivered codes against the chain\'s own float result times 255, over 8 x 8 blocks of the 2x output.', '',
                  '| dither | worst block-mean error, codes | mean error, codes |', '|---|---|---|']
        for mode, c in r['modes'].items():
            lines.append('| {} | {:.3f} | {:.4f} |'.format(mode, c['worst_block_mean_codes'], c['mean_codes']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'streams', 'ramp', 'summary'])
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
        args.rounds = {'kernel': 7}.get(args.mode, 2)
    {'kernel': kernel, 'streams': streams, 'ramp': ramp, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
