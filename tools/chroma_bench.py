#!/usr/bin/env python
"""Luma-only chains on 4:2:0 planes and frames handed out as views (measurement tool; results: profiles/chroma/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/chroma_bench.py kernel [--rounds 7] [--reps 50] [--out FILE.json]
    python tools/chroma_bench.py cost   [--root DIR] [--models a4,a2] [--frames 24] [--warmup 4] [--rounds 2] [--out FILE.json]
    python tools/chroma_bench.py off PARENT_TREE [--models ..] [--frames ..] [--rounds 3] [--limit 300] [--out FILE.json]
    python tools/chroma_bench.py gain   [--models ..] [--frames ..] [--warmup ..] [--rounds 3] [--out FILE.json]
    python tools/chroma_bench.py summary DIR          (DIR holds kernel.json / off.json / gain.json: whichever exist are written up as DIR/summary.md)

kernel  one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/planes_bench.py):
        A = resize_kernel_codes on the two 3840 x 2160 chroma planes of an 8K frame (source 2 x 540 x 960, scale 4, bicubic, depth 10 -> 10);
        B = stitch_planes_kernel on the same two planes at depth 10 (the chroma plan (2, 540, 960) x4, tiles of 256, fp16 canvas rounding): the fold the new kernel
        replaces on the luma-only path.  Gate: A's median <= B's median + B's own round-to-round spread.  Bytes per second from the bytes each must move
        (A: 2 h w reads + 2 (4h)(4w) writes of 2 bytes; B: 4-byte pool reads + 2-byte writes per sample).
cost    the planar streams (1080p yuv420p10le in and out, ring depth 2, distinct noise frames) with NO new key, through genFrameStream in one process; --root: the tree
        whose package is measured, so that the same file measures a checkout of the parent commit
off     `cost` of PARENT_TREE and of this tree as alternating child processes (the method of tools/reuse_bench.py versus), each child under its own time limit, nothing
        started after one that failed.  Gate: this tree's median frames per second within the parent's own leg-to-leg spread
gain    the same streams in four configurations -- chroma 'net' / 'bicubic', each with views off / on -- alternating `rounds` times in one process: frames per second
        and the ring's per-stage times (compute stage, tobytes_ms, ..) per leg

a4 uses the synthetic weights of tests/golden_defs.py (as bench.py does); every kernel's time is independent of the data."""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CROP, FMT, DEPTH = 1080, 1920, 256, 'yuv420p10le', 2


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
    import ctypes
    import torch
    from moephoto_amd import _lib, pixfmt
    from moephoto_amd.imageProcess import TilePlan
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    h, w, scale = H // 2, W // 2, 4
    (ox, cx), taps = pixfmt.chromaTable('bicubic', scale, 'center'), 4
    flat = [c for r in cx for c in r]
    tabs = ((ctypes.c_int16 * len(flat))(*flat), (ctypes.c_int8 * scale)(*ox))
    src = torch.randint(0, 1024, (2 * h * w,), dtype=torch.int16, device=dev)
    px = 2 * h * scale * w * scale
    out = torch.empty((px,), dtype=torch.int16, device=dev)
    pl = TilePlan((2, h, w), 1 << 40, 1e-3, 5, scale, 8, CROP)
    assert (pl.outH, pl.outW) == (h * scale, w * scale)
    pool = torch.rand(pl.pool_elems(2), dtype=torch.float32, device=dev)
    cases = {'A_resize_kernel_codes': lambda: _lib.check(L.moe_chroma_resample(src.data_ptr(), 10, h, w, out.data_ptr(), 10, scale, taps, tabs[0], tabs[1], tabs[0], tabs[1], 0, st)),
             'B_stitch_planes_kernel': lambda: _lib.check(L.moe_stitch_planes(pl._h, 0, pool.data_ptr(), None, 2, _lib.F16, 10, out.data_ptr(), st))}
    moved = {'A_resize_kernel_codes': 2 * (2 * h * w) + 2 * px, 'B_stitch_planes_kernel': px * (4 + 2)}

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
    a, b = res['A_resize_kernel_codes'], res['B_stitch_planes_kernel']
    a['bar_us'] = round(b['median_us'] + b['spread_us'], 2)
    a['holds'] = a['median_us'] <= a['bar_us']
    _emit({'planes': '2 x {} x {} from 2 x {} x {}, scale {}, bicubic, depth 10'.format(h * scale, w * scale, h, w, scale), 'reps': args.reps, 'rounds': args.rounds,
           'timing': 'device events around `reps` back-to-back launches', 'cases': res}, args.out)


def _setup(root):
    _path(root)
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_chroma_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    return tmp


def _steps(key, **source):
    return [dict({'op': 'buffer', 'pixFmt': FMT}, **source), {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}]


def _frames(n):
    import numpy as np
    from moephoto_amd import pixfmt
    rng = np.random.default_rng(2024)
    return [rng.integers(0, 1 << 10, pixfmt.frameBytes(FMT, W, H) // 2, dtype=np.uint16).tobytes() for _ in range(n)]


def _leg(stream, frames, warmup):
    """warmup untimed frames, then the rest between two host clock reads, the second behind a device synchronise -> (fps, the ring's stage ms per frame)"""
    import torch
    from moephoto_amd import procedure
    sink = {'bytes': 0}

    def write(buf):
        sink['bytes'] += len(buf)

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
    n = len(frames) - warmup
    dt = run(b''.join(frames[warmup:]), n)
    return round(n / dt, 3), {k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'}


def _legs(procedure, key, configs, frames, args):
    res = {name: {'fps': [], 'stage_ms_per_frame': []} for name in configs}
    for _ in range(args.rounds):
        for name, (source, kw) in configs.items():
            stream = procedure.genFrameStream(_steps(key, **source), W, H, DEPTH, timing=True, **kw)
            fps, stages = _leg(stream, frames, args.warmup)
            stream.close()
            res[name]['fps'].append(fps)
            res[name]['stage_ms_per_frame'].append(stages)
    for r in res.values():
        r['fps_median'] = median(r['fps'])
        for k in ('compute_ms', 'tobytes_ms', 'd2h_ms', 'h2d_ms', 'memcpy_ms'):
            r[k + '_median'] = median([s[k] for s in r['stage_ms_per_frame']])
    return res


def cost(args):
    root = os.path.abspath(args.root or HERE)
    tmp = _setup(root)
    from moephoto_amd import procedure
    frames = _frames(args.warmup + args.frames)
    result = {'root': root, 'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'models': {}}
    for key in args.models.split(','):
        result['models'][key] = _legs(procedure, key, {'plain': ({}, {})}, frames, args)['plain']
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def off(args):
    parent = os.path.abspath(args.parent)
    legs = []
    for r in range(args.rounds):
        for name, root in (('parent', parent), ('tree', HERE)):
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), 'cost', '--root', root, '--models', args.models,
                   '--frames', str(args.frames), '--warmup', str(args.warmup), '--rounds', '1' if name == 'tree' else '2']
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit('chroma_bench off: the {} child of round {} ended with status {}; nothing more is started'.format(name, r, p.returncode))
            legs.append((name, json.loads(p.stdout.strip().splitlines()[-1])))
    out = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'order': [n for n, _ in legs], 'models': {}}
    for key in args.models.split(','):
        m = {}
        for who in ('parent', 'tree'):
            got = [res['models'][key] for n, res in legs if n == who]
            m[who] = {'fps': sum((g['fps'] for g in got), []), 'compute_ms': [s['compute_ms'] for g in got for s in g['stage_ms_per_frame']]}
            m[who]['fps_median'], m[who]['compute_ms_median'] = median(m[who]['fps']), median(m[who]['compute_ms'])
        p = m['parent']
        m['parent_spread'] = {'fps': round(max(p['fps']) - min(p['fps']), 3), 'compute_ms': round(max(p['compute_ms']) - min(p['compute_ms']), 3)}
        m['tree_against_parent'] = {'fps': round(m['tree']['fps_median'] - p['fps_median'], 3), 'compute_ms': round(m['tree']['compute_ms_median'] - p['compute_ms_median'], 3)}
        m['holds'] = bool(-m['tree_against_parent']['fps'] <= m['parent_spread']['fps'])
        out['models'][key] = m
    _emit(out, args.out)


def gain(args):
    tmp = _setup(HERE)
    from moephoto_amd import procedure
    frames = _frames(args.warmup + args.frames)
    configs = {'net': ({'chroma': 'net'}, {}), 'net_views': ({'chroma': 'net'}, {'views': True}),
               'bicubic': ({'chroma': 'bicubic'}, {}), 'bicubic_views': ({'chroma': 'bicubic'}, {'views': True})}
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'models': {}}
    for key in args.models.split(','):
        result['models'][key] = _legs(procedure, key, configs, frames, args)
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.parent)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, o, g = load('kernel.json'), load('off.json'), load('gain.json')
    lines = ['# Luma-only chains and frames as views: measurements (`tools/chroma_bench.py`)', '',
             'MI355X, one device.  Streams: 1080p `yuv420p10le` in and out, ring depth 2, distinct noise frames.  Everything below is written by `chroma_bench.py summary`',
             'from the JSON files in this directory; a part whose file is missing was not measured.', '']
    lines += ['## Kernel gate: `resize_kernel_codes` against the fold it replaces', '']
    if k:
        a, b = k['cases']['A_resize_kernel_codes'], k['cases']['B_stitch_planes_kernel']
        lines += [k['planes'] + '; ' + k['timing'] + ', {} rounds of {} launches, the two legs alternating in one process.'.format(k['rounds'], k['reps']), '',
                  '| leg | median µs | fastest | spread over rounds | bytes moved | GB/s |', '|---|---|---|---|---|---|']
        for name, r in (('A `resize_kernel_codes<u16, u16, 4>`', a), ('B `stitch_planes_kernel<u16>` (C = 2)', b)):
            lines.append('| {} | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['bytes'], r['GB_per_s']))
        lines += ['', 'Gate (A <= B + B\'s spread = {} µs): **{}**.'.format(a['bar_us'], 'holds' if a['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## No cost when off: the planar streams with no new key, against the parent commit', '']
    if o:
        lines += ['Alternating child processes ({}), {} timed frames per leg after {} warm-up frames.'.format(', '.join(o['order']), o['frames'], o['warmup']), '',
                  '| stream | parent fps (legs) | median | tree fps (legs) | median | parent\'s spread | tree - parent | within |', '|---|---|---|---|---|---|---|---|']
        for key, m in o['models'].items():
            lines.append('| {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, m['parent']['fps'], m['parent']['fps_median'], m['tree']['fps'], m['tree']['fps_median'],
                                                                         m['parent_spread']['fps'], m['tree_against_parent']['fps'], 'yes' if m['holds'] else 'NO'))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## The gain: chroma `net` / `bicubic`, views off / on', '']
    if g:
        lines += ['One process, the four configurations alternating {} times, {} timed frames per leg after {} warm-up frames; medians over the legs, stage times in ms per frame.'.format(
            g['rounds'], g['frames'], g['warmup']), '', '| stream | configuration | fps (legs) | fps median | compute | tobytes | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|']
        for key, m in g['models'].items():
            for name, r in m.items():
                lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r['fps'], r['fps_median'], r['compute_ms_median'], r['tobytes_ms_median'],
                                                                                  r['d2h_ms_median'], r['h2d_ms_median'], r['memcpy_ms_median']))
        lines.append('')
        for key, m in g['models'].items():
            r = m['bicubic_views']
            stages = {s: r[s + '_ms_median'] for s in ('compute', 'tobytes', 'd2h', 'h2d', 'memcpy')}
            host = stages['memcpy'] + stages['tobytes']
            bound = max(list(stages.items()) + [('host thread (memcpy + tobytes)', host)], key=lambda kv: kv[1])
            lines.append('{}: with `bicubic` and views the frame time is {:.2f} ms ({} fps); the largest stage is {} at {:.2f} ms per frame.'.format(
                key, 1e3 / r['fps_median'], r['fps_median'], bound[0], bound[1]))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'cost', 'off', 'gain', 'summary'])
    ap.add_argument('parent', nargs='?')
    ap.add_argument('--root')
    ap.add_argument('--models', default='a4,a2')
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--limit', type=int, default=300)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.mode in ('off', 'summary') and not args.parent:
        ap.error(args.mode + ' needs a directory')
    if args.rounds is None:
        args.rounds = {'kernel': 7, 'cost': 2}.get(args.mode, 3)
    {'kernel': kernel, 'cost': cost, 'off': off, 'gain': gain, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
