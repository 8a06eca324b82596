#!/usr/bin/env python
"""Luma-guided chroma (measurement tool; results: profiles/guided/summary.md and the JSON files beside it).  kernel, gain and off need a GPU.

    python tools/guided_bench.py quality [--out FILE.json]
    python tools/guided_bench.py kernel [--rounds 7] [--reps 50] [--out FILE.json]
    python tools/guided_bench.py gain   [--models a4,a2] [--frames 24] [--warmup 4] [--rounds 3] [--out FILE.json]
    python tools/guided_bench.py off PARENT_TREE [--models ..] [--frames ..] [--rounds 3] [--limit 300] [--out FILE.json]
    python tools/guided_bench.py summary DIR          (DIR holds quality.json / kernel.json / gain.json / off.json: whichever exist are written up as DIR/summary.md)

quality the four scenes of tests/test_guided_cpu.py on the definition (no device): mean absolute error in 10-bit codes of pixfmt.resampleChroma 'bicubic' and of
        pixfmt.guidedChroma fed the true high-resolution Y', against the scene's own chroma at the output's size; scales 2, 3, 4, both sitings
kernel  one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/chroma_bench.py):
        A = resize_kernel_guided and B = resize_kernel_codes (bicubic), both writing the two 3840 x 2160 chroma planes of an 8K frame (source 2 x 540 x 960, scale 4,
        depth 10 -> 10).  Bytes per second from the bytes each must move (B: the source chroma and the output chroma; A: those, the source luma and the output luma).
gain    the planar streams (1080p yuv420p10le in and out, ring depth 2, distinct noise frames) with 'chroma' = 'net' / 'bicubic' / 'guided', alternating `rounds`
        times in one process: frames per second and the ring's per-stage times.  Gate, on the a4 stream's compute stage: 'guided' keeps at least half of the
        gain 'bicubic' has over 'net'
off     the streams with NO 'chroma' key in PARENT_TREE and in this tree as alternating child processes: tools/chroma_bench.py's `off`, as it is

a4 uses the synthetic weights of tests/golden_defs.py (as bench.py does); every kernel's time is independent of the data."""
import argparse
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
import chroma_bench as cb          # noqa: E402  (the stream legs, the frames and the parent-against-tree method are that tool's)

median, H, W = cb.median, cb.H, cb.W


def quality(args):
    cb._path(HERE)
    import numpy as np
    import test_guided_cpu as t
    from moephoto_amd import pixfmt
    fmt, rows = 'yuv420p10le', []
    for name in ('edge', 'text', 'smooth', 'iso'):
        rng = np.random.default_rng(20)          # (the test's seed and order of draws: these are the test's numbers)
        for s in (2, 3, 4):
            for loc in t.LOCS:
                Ys, C = t._sceneFrame(name, 1, loc, rng)
                Yo, truth = t._sceneFrame(name, s, loc, rng)
                mae = lambda got: float(np.abs(got.astype(np.int64) - truth).mean())
                b, g = mae(pixfmt.resampleChroma(C, fmt, fmt, s, 'bicubic', loc)), mae(pixfmt.guidedChroma(C, Ys, Yo, fmt, fmt, s, loc))
                rows.append({'scene': name, 'scale': s, 'loc': loc, 'bicubic_mae': round(b, 3), 'guided_mae': round(g, 3), 'ratio': round(g / b, 3), 'bound': t.QUALITY[name]})
    cb._emit({'source_luma': [t.QH, t.QW], 'rows': rows, 'holds': all(r['ratio'] <= r['bound'] for r in rows)}, args.out)


def kernel(args):
    cb._path(HERE)
    import ctypes
    import torch
    from moephoto_amd import _lib, pixfmt
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    h, w, scale = H // 2, W // 2, 4
    flat = lambda rows: [c for r in rows for c in r]
    (ox, cx) = pixfmt.chromaTable('bicubic', scale, 'center')
    tabs = ((ctypes.c_int16 * (4 * scale))(*flat(cx)), (ctypes.c_int8 * scale)(*ox))
    (gox, gcx) = pixfmt.guidedTable(scale, 'center')
    gtabs = ((ctypes.c_uint8 * (4 * scale))(*flat(gcx)), (ctypes.c_int8 * scale)(*gox), (ctypes.c_uint8 * 64)(*pixfmt.guidedRange()))
    src = torch.randint(0, 1024, (6 * h * w,), dtype=torch.int16, device=dev)                          # a source frame: Y, Cb, Cr
    px = 2 * h * scale * w * scale
    out = torch.randint(0, 1024, (3 * px,), dtype=torch.int16, device=dev)                             # an output frame: Y (noise: every range weight occurs), Cb, Cr
    at_c, at_oc = src.data_ptr() + 4 * h * w * 2, out.data_ptr() + 2 * px * 2
    cases = {'A_resize_kernel_guided': lambda: _lib.check(L.moe_chroma_guided(at_c, src.data_ptr(), 10, h, w, at_oc, out.data_ptr(), 10, scale, 0, gtabs[0], gtabs[1],
                                                                              gtabs[0], gtabs[1], gtabs[2], 0, st)),
             'B_resize_kernel_codes': lambda: _lib.check(L.moe_chroma_resample(at_c, 10, h, w, at_oc, 10, scale, 4, tabs[0], tabs[1], tabs[0], tabs[1], 0, st))}
    moved = {'A_resize_kernel_guided': 2 * (6 * h * w) + 2 * (3 * px), 'B_resize_kernel_codes': 2 * (2 * h * w) + 2 * px}

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
    res['ratio_A_over_B'] = round(res['A_resize_kernel_guided']['median_us'] / res['B_resize_kernel_codes']['median_us'], 2)
    cb._emit({'planes': '2 x {} x {} from 2 x {} x {}, scale {}, depth 10, noise luma'.format(h * scale, w * scale, h, w, scale), 'reps': args.reps, 'rounds': args.rounds,
              'timing': 'device events around `reps` back-to-back launches', 'cases': res}, args.out)


def gain(args):
    tmp = cb._setup(HERE)
    from moephoto_amd import procedure
    frames = cb._frames(args.warmup + args.frames)
    configs = {'net': ({'chroma': 'net'}, {}), 'bicubic': ({'chroma': 'bicubic'}, {}), 'guided': ({'chroma': 'guided'}, {})}
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'models': {}}
    for key in args.models.split(','):
        m = cb._legs(procedure, key, configs, frames, args)
        have, kept = m['net']['compute_ms_median'] - m['bicubic']['compute_ms_median'], m['net']['compute_ms_median'] - m['guided']['compute_ms_median']
        m['gate'] = {'bicubic_gain_ms': round(have, 3), 'guided_gain_ms': round(kept, 3), 'share_kept': round(kept / have, 3) if have > 0 else None,
                     'holds': bool(have > 0 and kept >= 0.5 * have)}
        result['models'][key] = m
    shutil.rmtree(tmp, ignore_errors=True)
    cb._emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.parent)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    q, k, g, o = load('quality.json'), load('kernel.json'), load('gain.json'), load('off.json')
    lines = ['# Luma-guided chroma: measurements (`tools/guided_bench.py`)', '',
             'Everything below is written by `guided_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '',
             '## Quality on the definition: guided against bicubic (no device)', '']
    if q:
        lines += ['The four scenes of `tests/test_guided_cpu.py` (source luma {} x {}, 10 bits, Y\' noise of sigma 0.004), mean absolute error in codes against the scene\'s own '
                  'chroma at the output\'s size; guided is fed the true high-resolution Y\'.'.format(q['source_luma'][1], q['source_luma'][0]), '',
                  '| scene | scale | siting | bicubic MAE | guided MAE | guided / bicubic | bound |', '|---|---|---|---|---|---|---|']
        lines += ['| {scene} | {scale} | {loc} | {bicubic_mae} | {guided_mae} | {ratio} | {bound} |'.format(**r) for r in q['rows']]
        lines += ['', 'Every bound holds: **{}**.'.format('yes' if q['holds'] else 'NO'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Kernel: `resize_kernel_guided` beside `resize_kernel_codes` (bicubic)', '']
    if k:
        lines += ['MI355X, one device.  ' + k['planes'] + '; ' + k['timing'] + ', {} rounds of {} launches, the two legs alternating in one process.'.format(k['rounds'], k['reps']), '',
                  '| leg | median µs | fastest | spread over rounds | bytes moved | GB/s |', '|---|---|---|---|---|---|']
        for name, key in (('A `resize_kernel_guided<u16, u16>`', 'A_resize_kernel_guided'), ('B `resize_kernel_codes<u16, u16, 4>`', 'B_resize_kernel_codes')):
            r = k['cases'][key]
            lines.append('| {} | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['bytes'], r['GB_per_s']))
        lines += ['', 'A / B = {}.'.format(k['cases']['ratio_A_over_B']), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: chroma `net` / `bicubic` / `guided`', '']
    if g:
        lines += ['MI355X, one device; 1080p `yuv420p10le` in and out, ring depth {}, distinct noise frames.  One process, the three configurations alternating {} times, {} timed '
                  'frames per leg after {} warm-up frames; medians over the legs, stage times in ms per frame.'.format(g['depth'], g['rounds'], g['frames'], g['warmup']), '',
                  '| stream | configuration | fps (legs) | fps median | compute | tobytes | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|']
        for key, m in g['models'].items():
            for name in ('net', 'bicubic', 'guided'):
                r = m[name]
                lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r['fps'], r['fps_median'], r['compute_ms_median'], r['tobytes_ms_median'],
                                                                                  r['d2h_ms_median'], r['h2d_ms_median'], r['memcpy_ms_median']))
        lines.append('')
        for key, m in g['models'].items():
            t = m['gate']
            lines.append('{}: on the compute stage `bicubic` gains {} ms per frame over `net`, `guided` {} ms: {} of it{}.'.format(
                key, t['bicubic_gain_ms'], t['guided_gain_ms'], t['share_kept'],
                ' -- gate (at least half, on a4): **{}**'.format('holds' if t['holds'] else 'MISSED') if key == 'a4' else ''))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## No cost when off: the planar streams with no `chroma` key, against the parent commit', '']
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
    ap.add_argument('mode', choices=['quality', 'kernel', 'gain', 'off', 'summary'])
    ap.add_argument('parent', nargs='?')
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
        args.rounds = 7 if args.mode == 'kernel' else 3
    {'quality': quality, 'kernel': kernel, 'gain': gain, 'off': cb.off, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
