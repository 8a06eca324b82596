#!/usr/bin/env python
"""Fitted sizes on RGB chains (measurement tool; results: profiles/fit_px/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/fit_px_bench.py edge    [--rounds 7] [--reps 30] [--out FILE.json]
    python tools/fit_px_bench.py streams [--models a4,a2] [--frames 12] [--warmup 4] [--rounds 2] [--out FILE.json]
    python tools/fit_px_bench.py summary DIR          (DIR holds edge.json / streams.json: whichever exist are written up as DIR/summary.md)

edge     the output edge alone of the a4 1080p chain whose resize step asks for 4K, from the same fp32 tile pool of the 8K plan, one process, `rounds` alternating
         rounds of `reps` back-to-back runs between device events, microseconds per run:
         A ('fit')    = moe_stitch_out (stitch_out_kernel: the fold writes the 16-bit samples of 7680 x 4320 x 3) + moe_fit_run (resize_kernel_fit_px -> 3840 x 2160 x 3
                        bgr48le samples, bicubic);
         B ('method') = moe_stitch (the fold writes the fp16 canvas 3 x 4320 x 7680) + moe_resize (bicubic -> 3 x 2160 x 3840) + moe_to_output (16 bits).
         Gate: A's median <= B's median.  Each leg's kernels are also timed one by one, and resize_kernel_fit_px alone at 8 bits out and at 3/2 up from 4K.
streams  bgr48le streams whose resize step names the size with 'fit' beside the same step with 'method', alternating `rounds` times in one process: a4, 1080p -> 4K
         (from 8K) and a2, 720p -> 1080p, each with and without 'chroma': 'bicubic' on the SR step; frames per second and the ring's compute-stage ms per frame.

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


def edge(args):
    _path(HERE)
    import torch
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import TilePlan, fitPixels
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    H8, W8, H4, W4 = 4320, 7680, 2160, 3840
    pl = TilePlan((3, 1080, 1920), 1 << 40, 1e-3, 5, 4, 8, CROP)
    assert (pl.outH, pl.outW) == (H8, W8)
    pool = torch.rand(pl.pool_elems(3), dtype=torch.float32, device=dev)
    flat = lambda t: t.view(torch.uint8).reshape(-1)
    samples8k = torch.empty((H8, W8, 3), dtype=torch.int16, device=dev)
    frame16, frame8 = torch.empty((H4, W4, 3), dtype=torch.int16, device=dev), torch.empty((H4, W4, 3), dtype=torch.uint8, device=dev)
    canvas = torch.empty((3, H8, W8), dtype=torch.float16, device=dev)
    small = torch.empty((3, H4, W4), dtype=torch.float16, device=dev)
    fit16, fit8 = fitPixels(16, 16, 3, H8, W8, H4, W4, 'bicubic'), fitPixels(16, 8, 3, H8, W8, H4, W4, 'bicubic')
    up_src, up_dst = torch.empty((H4, W4, 3), dtype=torch.int16, device=dev), torch.empty((H4 * 3 // 2, W4 * 3 // 2, 3), dtype=torch.int16, device=dev)
    fit_up = fitPixels(16, 16, 3, H4, W4, H4 * 3 // 2, W4 * 3 // 2, 'bicubic')

    stitch_out = lambda: _lib.check(L.moe_stitch_out(pl._h, 0, pool.data_ptr(), None, 3, _lib.F16, 16, samples8k.data_ptr(), _lib.U16, st))
    fit = lambda: fit16(flat(samples8k), flat(frame16))
    stitch = lambda: _lib.check(L.moe_stitch(pl._h, 0, pool.data_ptr(), None, 3, canvas.data_ptr(), _lib.F16, st))
    resize = lambda: _lib.check(L.moe_resize(canvas.data_ptr(), small.data_ptr(), _lib.F16, 3, H8, W8, H4, W4, _lib.RESIZE_MODES['bicubic'], 0, st))
    quantise = lambda: _lib.check(L.moe_to_output(small.data_ptr(), _lib.F16, H4, W4, 3, 16, frame16.data_ptr(), _lib.U16, 0, st))
    cases = {'A_fit_edge': lambda: (stitch_out(), fit()), 'B_method_edge': lambda: (stitch(), resize(), quantise()),
             'A1_stitch_out_16': stitch_out, 'A2_resize_kernel_fit_px': fit, 'B1_stitch_canvas': stitch, 'B2_moe_resize': resize, 'B3_moe_to_output': quantise,
             'fit_px_8K_to_4K_8_bits': lambda: fit8(flat(samples8k), flat(frame8)), 'fit_px_4K_up_3_2': lambda: fit_up(flat(up_src), flat(up_dst))}
    flat(samples8k).random_(0, 256)
    flat(up_src).random_(0, 256)

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
    res = {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2)} for k, v in rounds.items()}
    for k, f in (('A2_resize_kernel_fit_px', fit16), ('fit_px_8K_to_4K_8_bits', fit8), ('fit_px_4K_up_3_2', fit_up)):
        info = f.info(dev)
        res[k]['tile'], res[k]['lds_bytes'] = list(info['tile']), info['lds']
    a, b = res['A_fit_edge'], res['B_method_edge']
    a['bar_us'] = b['median_us']
    a['holds'] = a['median_us'] <= a['bar_us']
    _emit({'reps': args.reps, 'rounds': args.rounds, 'timing': 'device events around `reps` back-to-back runs', 'cases': res}, args.out)


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
    tmp = tempfile.mkdtemp(prefix='moe_fit_px_bench_')
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
    from moephoto_amd import procedure
    rng = np.random.default_rng(2024)
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'streams': {}}
    for key, (w, h), (W, H) in (('a4', (1920, 1080), (3840, 2160)), ('a2', (1280, 720), (1920, 1080))):
        if key not in args.models.split(','):
            continue
        n = args.frames + args.warmup
        frames = [rng.integers(0, 65536, w * h * 3, dtype=np.uint16).tobytes() for _ in range(n)]
        configs = {}
        for chroma in (None, 'bicubic'):
            sr = dict({'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}, **({'chroma': chroma} if chroma else {}))
            for way in ('fit', 'method'):
                configs['{}_{}'.format('luma_bicubic' if chroma else 'net', way)] = [{'op': 'buffer', 'bitDepth': 16}, dict(sr), {'op': 'resize', 'width': W, 'height': H, way: 'bicubic'}]
        res = {name: {'fps': [], 'compute_ms': []} for name in configs}
        for _ in range(args.rounds):
            for name, steps in configs.items():
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
    e, s = load('edge.json'), load('streams.json')
    lines = ['# Fitted sizes on RGB chains: measurements (`tools/fit_px_bench.py`)', '',
             'MI355X, one device.  Everything below is written by `fit_px_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '']
    lines += ['## Edge gate: the fold to 16-bit samples + `resize_kernel_fit_px` against the canvas fold + `moe_resize` + `moe_to_output`', '']
    if e:
        lines += ['The a4 1080p chain\'s 8K tile pool -> a 3840 x 2160 bgr48le frame, bicubic; ' + e['timing'] + ', {} rounds of {} runs, the legs alternating in one process.'.format(
            e['rounds'], e['reps']), '', '| leg | median µs | fastest | spread over rounds | tile | LDS bytes |', '|---|---|---|---|---|---|']
        for name, r in e['cases'].items():
            lines.append('| `{}` | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], 'x'.join(map(str, r['tile'])) if 'tile' in r else '', r.get('lds_bytes', '')))
        a = e['cases']['A_fit_edge']
        lines += ['', 'Gate (A <= B = {} µs): **{}**.'.format(a['bar_us'], 'holds' if a['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: `\'fit\'` against `\'method\'` on the resize step of a bgr48le chain', '']
    if s:
        lines += ['Ring depth {}, distinct noise frames, {} timed frames per leg after {} warm-up frames, the configurations alternating {} times in one process.'.format(
            s['depth'], s['frames'], s['warmup'], s['rounds']), '', '| stream | configuration | edge | fps (legs) | fps median | compute ms (legs) | median |', '|---|---|---|---|---|---|---|']
        for key, m in s['streams'].items():
            for name, r in m.items():
                lines.append('| {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r.get('edge', ''), r['fps'], r['fps_median'], r['compute_ms'], r['compute_ms_median']))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['edge', 'streams', 'summary'])
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--models', default='a4,a2')
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.mode == 'summary' and not args.dir:
        ap.error('summary needs a directory')
    if args.rounds is None:
        args.rounds = 7 if args.mode == 'edge' else 2
    {'edge': edge, 'streams': streams, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
