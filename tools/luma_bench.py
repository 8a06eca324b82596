#!/usr/bin/env python
"""Luma-only SR / DN steps on RGB sources (measurement tool; results: profiles/luma/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/luma_bench.py kernel  [--rounds 7] [--reps 30] [--out FILE.json]
    python tools/luma_bench.py frame   [--rounds 5] [--reps 8] [--out FILE.json]
    python tools/luma_bench.py streams [--models a4,a2] [--frames 16] [--warmup 4] [--rounds 2] [--out FILE.json]
    python tools/luma_bench.py diff    [--out FILE.json]
    python tools/luma_bench.py summary DIR          (DIR holds kernel.json / frame.json / streams.json / diff.json / oracle.json: whichever exist are written up as DIR/summary.md)

kernel   the a4 1080p -> 8K geometry, one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch:
         to_float_luma_kernel on the fp16 (3, 1080, 1920) frame; the fp32 moe_resize (bicubic) of its chroma pair to 4320 x 7680; stitch_luma_kernel in sample form at
         16 bits on the plan (1, 1080, 1920) x4 with tiles of 256; and the parent's stitch_out_kernel (C = 3, 16 bits) on the plan (3, 1080, 1920) -- the fold the new
         edge replaces.  Gate: stitch_luma's median <= stitch_out's median + stitch_out's own round-to-round spread.
frame    a4 1080p -> 8K, fp16 I/O, default arithmetic, the frame's compute alone (image on the device -> the encoder's 16-bit samples on the device): doCropLuma
         ('bicubic') against doCropOut on the three planes, alternating in one process; and the split and the resize alone, for the expectation
         T_luma <= 1.25 T_rgb / 3 + t_split + t_resize.
streams  bgr48le 1080p frames through genFrameStream (ring depth 2, distinct noise frames), each model with and without 'chroma': 'bicubic', frames handed out as
         copies and as views (an 8K bgr48le frame is 199 MB: its copy is the host's largest stage), alternating: frames per second and the ring's per-stage times.
diff     informational: maximum and mean absolute difference between the luma-only and the RGB chain's result (a2 and a4, fp16, a natural and a noise frame of
         540 x 960) -- a different algorithm, not an error.

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
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import TilePlan
    _lib.require_device()
    L, dev, st = _lib.lib(), torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream
    x = torch.rand((3, H, W), device=dev).half()
    y, c = torch.empty((1, H, W), dtype=torch.float16, device=dev), torch.empty((2, H, W), dtype=torch.float32, device=dev)
    C = torch.empty((2, 4 * H, 4 * W), dtype=torch.float32, device=dev)
    out = torch.empty((4 * H, 4 * W, 3), dtype=torch.int16, device=dev)
    p1, p3 = TilePlan((1, H, W), 1 << 40, 1e-3, 5, 4, 8, CROP), TilePlan((3, H, W), 1 << 40, 1e-3, 5, 4, 8, CROP)
    pool1, pool3 = torch.rand(p1.pool_elems(1), device=dev), torch.rand(p3.pool_elems(3), device=dev)
    cases = {'to_float_luma_kernel': lambda: _lib.check(L.moe_luma_split(x.data_ptr(), _lib.F16, 3, x.stride(0), x.stride(1), 1, H, W, 0, 0, y.data_ptr(), c.data_ptr(), 0, st)),
             'resize_chroma_fp32': lambda: _lib.check(L.moe_resize(c.data_ptr(), C.data_ptr(), _lib.F32, 2, H, W, 4 * H, 4 * W, 2, 0, st)),
             'stitch_luma_kernel': lambda: _lib.check(L.moe_stitch_luma(p1._h, 0, pool1.data_ptr(), None, 1, _lib.F16, C.data_ptr(), 0, 0, 16, out.data_ptr(), _lib.U16, st)),
             'stitch_out_kernel_C3': lambda: _lib.check(L.moe_stitch_out(p3._h, 0, pool3.data_ptr(), None, 3, _lib.F16, 16, out.data_ptr(), _lib.U16, st))}
    res = _alternate(cases, args.rounds, args.reps)
    px = 16 * H * W
    moved = {'to_float_luma_kernel': H * W * (3 * 2 + 2 + 8), 'resize_chroma_fp32': 2 * 4 * (H * W + px), 'stitch_luma_kernel': px * (4 + 8 + 6), 'stitch_out_kernel_C3': px * (12 + 6)}
    for k, r in res.items():
        r['bytes'], r['GB_per_s'] = moved[k], round(moved[k] / r['median_us'] / 1e3, 1)
    a, b = res['stitch_luma_kernel'], res['stitch_out_kernel_C3']
    a['bar_us'] = round(b['median_us'] + b['spread_us'], 2)
    a['holds'] = a['median_us'] <= a['bar_us']
    _emit({'geometry': 'a4 1080p -> 8K: (1 | 3, 1080, 1920) x4, tiles of 256, fp16 canvas rounding, 16-bit samples', 'reps': args.reps, 'rounds': args.rounds,
           'timing': 'device events around `reps` back-to-back launches', 'cases': res}, args.out)


def _setup():
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_luma_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    return tmp


def frame(args):
    tmp = _setup()
    import torch
    from moephoto_amd import imageProcess as ip, runSR
    dev = torch.device('cuda:0')
    opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 4, 'ensemble': 0})
    x = torch.rand((3, H, W), device=dev).half()
    out = torch.empty((4 * H, 4 * W, 3), dtype=torch.int16, device=dev)
    split = ip.lumaSplit('bt709', 'bgr')
    _, c = split(x)
    cases = {'T_rgb_doCropOut': lambda: ip.doCropOut(opt, x, 16, out), 'T_luma_doCropLuma': lambda: ip.doCropLuma(opt, x, 'bicubic', 'bt709', 'bgr', 16, out),
             't_split': lambda: split(x), 't_resize': lambda: ip.resizeByTorch(c, 4 * W, 4 * H, 'bicubic')}
    res = _alternate(cases, args.rounds, args.reps)
    rgb, lum = res['T_rgb_doCropOut']['median_us'], res['T_luma_doCropLuma']['median_us']
    bound = 1.25 * rgb / 3 + res['t_split']['median_us'] + res['t_resize']['median_us']
    shutil.rmtree(tmp, ignore_errors=True)
    _emit({'workload': 'a4 1080p -> 8K, fp16 I/O, default arithmetic, tiles of 256: image on the device -> 16-bit samples on the device', 'reps': args.reps, 'rounds': args.rounds,
           'cases': res, 'T_luma_us': lum, 'T_rgb_us': rgb, 'expectation_us': round(bound, 1), 'ratio_luma_to_rgb': round(lum / rgb, 4),
           'ratio_luma_to_expectation': round(lum / bound, 4), 'holds': lum <= bound}, args.out)


def _leg(stream, frames, warmup):
    import torch
    from moephoto_amd import procedure
    sink = {'bytes': 0}

    def run(data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(stream, io.BytesIO(data).read, lambda buf: sink.__setitem__('bytes', sink['bytes'] + len(buf)))
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0
    if warmup:
        run(b''.join(frames[:warmup]), warmup)
    st = stream.backend.stats
    for k in st:
        st[k] = 0
    n = len(frames) - warmup
    dt = run(b''.join(frames[warmup:]), n)
    return round(n / dt, 3), {k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'}


def streams(args):
    tmp = _setup()
    import numpy as np
    from moephoto_amd import procedure
    rng = np.random.default_rng(2024)
    frames = [rng.integers(0, 65536, H * W * 3, dtype=np.uint16).tobytes() for _ in range(args.warmup + args.frames)]
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'source': 'bgr48le 1080p', 'models': {}}
    for key in args.models.split(','):
        res = {name: {'fps': [], 'stage_ms_per_frame': []} for name in ('net', 'bicubic', 'net_views', 'bicubic_views')}
        for _ in range(args.rounds):
            for name in res:
                step = {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}
                if not name.startswith('net'):
                    step['chroma'] = 'bicubic'
                stream = procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, step], W, H, DEPTH, timing=True, views=name.endswith('_views'))
                fps, stages = _leg(stream, frames, args.warmup)
                stream.close()
                res[name]['fps'].append(fps)
                res[name]['stage_ms_per_frame'].append(stages)
        for r in res.values():
            r['fps_median'] = median(r['fps'])
            for k in ('compute_ms', 'tobytes_ms', 'd2h_ms', 'h2d_ms', 'memcpy_ms'):
                r[k + '_median'] = median([s[k] for s in r['stage_ms_per_frame']])
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def diff(args):
    tmp = _setup()
    import numpy as np
    import torch
    import golden_defs as gd
    from moephoto_amd import imageProcess as ip, runSR
    dev = torch.device('cuda:0')
    shape = (3, 540, 960)
    images = {'natural': gd.natural_image(101, shape), 'noise': gd.noise_image(7, shape)}
    result = {'shape': list(shape), 'io': 'fp16', 'chroma': 'bicubic, bt709', 'models': {}}
    for key in ('a2', 'a4'):
        opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': int(key[-1]), 'ensemble': 0})
        result['models'][key] = {}
        for name, im in images.items():
            x = torch.from_numpy(im).to(dev).half()
            a = ip.doCrop(opt, x).float().cpu().numpy()
            b = ip.doCropLuma(opt, x, 'bicubic', 'bt709', 'rgb').float().cpu().numpy()
            d = np.abs(a.astype(np.float64) - b)
            result['models'][key][name] = {'max_abs': float(d.max()), 'mean_abs': float(d.mean())}
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.dir)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, f, s, x, o = load('kernel.json'), load('frame.json'), load('streams.json'), load('diff.json'), load('oracle.json')
    lines = ['# Luma-only steps on RGB sources: measurements (`tools/luma_bench.py`)', '',
             'MI355X, one device.  Everything below is written by `luma_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '']
    lines += ['## Against the oracle', '']
    if o:
        lines += ['`tests/test_gpu_luma.py::test_an_image_through_a2_against_the_oracle` (fp32 I/O, a2, 100 x 140 noise, the definition with the oracle\'s doCrop on Y\'): '
                  'max |engine - definition| = {:.3e} (bound {:.3e}).'.format(o['max_abs'], o['bound']), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Kernels alone, on the a4 1080p -> 8K geometry', '']
    if k:
        lines += [k['geometry'] + '; ' + k['timing'] + ', {} rounds of {} launches, the legs alternating in one process.'.format(k['rounds'], k['reps']), '',
                  '| leg | median µs | fastest | spread over rounds | bytes moved | GB/s |', '|---|---|---|---|---|---|']
        for name, r in k['cases'].items():
            lines.append('| `{}` | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['bytes'], r['GB_per_s']))
        a = k['cases']['stitch_luma_kernel']
        lines += ['', 'Gate (`stitch_luma_kernel` <= `stitch_out_kernel` (C = 3) + its spread = {} µs): **{}**.'.format(a['bar_us'], 'holds' if a['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Frame time of a4 1080p -> 8K', '']
    if f:
        lines += [f['workload'] + '; {} rounds of {} frames per leg, alternating in one process, device events.'.format(f['rounds'], f['reps']), '',
                  '| leg | median µs | fastest | spread over rounds |', '|---|---|---|---|']
        for name, r in f['cases'].items():
            lines.append('| `{}` | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us']))
        lines += ['', 'T_luma = {} µs, T_rgb = {} µs: ratio {}.  Expectation 1.25 T_rgb / 3 + t_split + t_resize = {} µs: T_luma is {} of it -- **{}**.'.format(
            f['T_luma_us'], f['T_rgb_us'], f['ratio_luma_to_rgb'], f['expectation_us'], f['ratio_luma_to_expectation'], 'holds' if f['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: bgr48le 1080p with and without the key', '']
    if s:
        lines += ['Ring depth {}, {} timed frames per leg after {} warm-up frames, the configurations alternating {} times; stage times in ms per frame (`_views`: frames handed out as views, no host copy).'.format(
            s['depth'], s['frames'], s['warmup'], s['rounds']), '', '| stream | chroma | fps (legs) | fps median | compute | tobytes | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|']
        for key, m in s['models'].items():
            for name, r in m.items():
                lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r['fps'], r['fps_median'], r['compute_ms_median'], r['tobytes_ms_median'],
                                                                                  r['d2h_ms_median'], r['h2d_ms_median'], r['memcpy_ms_median']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## Difference from the RGB chain (informational: a different algorithm)', '']
    if x:
        lines += ['a2 carries the zoo\'s weights, a4 the synthetic ones (its numbers say nothing about a trained net).  {} frames, {} I/O, chroma {}.'.format(' x '.join(str(v) for v in x['shape']), x['io'], x['chroma']), '', '| model | frame | max abs | mean abs |', '|---|---|---|---|']
        for key, m in x['models'].items():
            for name, r in m.items():
                lines.append('| {} | {} | {:.4f} | {:.6f} |'.format(key, name, r['max_abs'], r['mean_abs']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'frame', 'streams', 'diff', 'summary'])
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--models', default='a4,a2')
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.mode == 'summary' and not args.dir:
        ap.error('summary needs a directory')
    if args.rounds is None:
        args.rounds = {'kernel': 7, 'frame': 5}.get(args.mode, 2)
    if args.reps is None:
        args.reps = {'kernel': 30}.get(args.mode, 8)
    {'kernel': kernel, 'frame': frame, 'streams': streams, 'diff': diff, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
