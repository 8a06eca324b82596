#!/usr/bin/env python
"""RGB frames from chains on 4:2:0 planes (measurement tool; results: profiles/planes_rgb/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/planes_rgb_bench.py kernel [--rounds 7] [--reps 50] [--out FILE.json]
    python tools/planes_rgb_bench.py gain   [--models a4,a2] [--frames 24] [--warmup 4] [--rounds 3] [--out FILE.json]
    python tools/planes_rgb_bench.py off PARENT_TREE [--models ..] [--frames ..] [--rounds 3] [--limit 300] [--out FILE.json]
    python tools/planes_rgb_bench.py summary DIR          (DIR holds kernel.json / gain.json / off.json: whichever exist are written up as DIR/summary.md)

kernel  one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/chroma_bench.py):
        A = to_output_rgb420_kernel<u16, u16, 4> on an 8K yuv420p16le frame -> bgr48le (bicubic, centre siting); B = stitch_out_kernel<u16, 3, 4> on the a4 1080p -> 8K
        pool (tiles of 256, fp16 canvas rounding), which writes the same 199 MB.  Gate: A's median <= B's median + B's own round-to-round spread.  Bytes per second
        from the bytes each must move (A: 1.5 samples read and 3 written per pixel, 2 bytes each; B: 4-byte pool reads and 2-byte writes per sample).
gain    the 1080p streams (ring depth 2, distinct noise frames) in four forms -- bgr48le -> bgr48le; yuv420p10le -> yuv420p10le; yuv420p10le -> bgr48le with 'chroma'
        'net' and with 'bicubic' -- each with views off / on, alternating `rounds` times in one process: frames per second and the ring's per-stage times.  Gate, on the
        a4 stream's compute stage: yuv420p10le -> bgr48le ('net') keeps at least half of the gain yuv420p10le -> yuv420p10le has over bgr48le -> bgr48le
off     the planar streams with NO new key in PARENT_TREE and in this tree as alternating child processes: tools/chroma_bench.py's `off`, as it is

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
FORMS = ('rgb_rgb', 'yuv_yuv', 'yuv_rgb_net', 'yuv_rgb_bicubic')


def kernel(args):
    cb._path(HERE)
    import ctypes
    import torch
    from moephoto_amd import _lib, pixfmt
    from moephoto_amd.imageProcess import TilePlan
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    oh, ow = 4 * H, 4 * W
    (ox, cx) = pixfmt.chromaTable('bicubic', 2, 'center')
    flat = [c for r in cx for c in r]
    tabs = ((ctypes.c_int16 * 8)(*flat), (ctypes.c_int8 * 2)(*ox), (ctypes.c_int32 * 5)(*pixfmt.rgbCoefficients('bt709', 16, 16)))
    src = torch.randint(-32768, 32767, (oh * ow * 3 // 2,), dtype=torch.int16, device=dev)          # an 8K yuv420p16le frame: noise over all 16 bits
    out = torch.empty((oh * ow * 3,), dtype=torch.int16, device=dev)
    pl = TilePlan((3, H, W), 1 << 40, 1e-3, 5, 4, 8, cb.CROP)
    assert (pl.outH, pl.outW) == (oh, ow)
    pool = torch.rand(pl.pool_elems(3), dtype=torch.float32, device=dev)
    cases = {'A_to_output_rgb420_kernel': lambda: _lib.check(L.moe_planes_to_rgb(src.data_ptr(), 16, oh, ow, out.data_ptr(), 16, 0, 0, 4, tabs[0], tabs[1], tabs[0], tabs[1], tabs[2], 0, st)),
             'B_stitch_out_kernel': lambda: _lib.check(L.moe_stitch_out(pl._h, 0, pool.data_ptr(), None, 3, _lib.F16, 16, out.data_ptr(), _lib.U16, st))}
    moved = {'A_to_output_rgb420_kernel': 2 * (oh * ow * 3 // 2) + 2 * (3 * oh * ow), 'B_stitch_out_kernel': 3 * oh * ow * (4 + 2)}

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
    a, b = res['A_to_output_rgb420_kernel'], res['B_stitch_out_kernel']
    a['bar_us'] = round(b['median_us'] + b['spread_us'], 2)
    a['holds'] = a['median_us'] <= a['bar_us']
    cb._emit({'frame': '{} x {} yuv420p16le -> bgr48le, bicubic, centre siting, bt709'.format(ow, oh), 'reps': args.reps, 'rounds': args.rounds,
              'timing': 'device events around `reps` back-to-back launches', 'cases': res}, args.out)


def _form(key, form):
    """(steps, bytes of a source frame) of one form of the 1080p stream of model `key`."""
    from moephoto_amd import pixfmt
    sr = {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}
    if form == 'rgb_rgb':
        return [{'op': 'buffer', 'bitDepth': 16}, sr], W * H * 6
    source = dict({'op': 'buffer', 'pixFmt': cb.FMT}, **({'chroma': 'bicubic'} if form == 'yuv_rgb_bicubic' else {}))
    return [source, sr] + ([] if form == 'yuv_yuv' else [{'op': 'output', 'pixFmt': 'bgr48le'}]), pixfmt.frameBytes(cb.FMT, W, H)


def gain(args):
    tmp = cb._setup(HERE)
    import numpy as np
    from moephoto_amd import procedure
    rng = np.random.default_rng(2024)
    noise = {n: [rng.integers(0, 1 << 10, n // 2, dtype=np.uint16).tobytes() for _ in range(args.warmup + args.frames)] for n in {_form('a4', f)[1] for f in FORMS}}
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'models': {}}
    for key in args.models.split(','):
        res = {f + v: {'fps': [], 'stage_ms_per_frame': []} for f in FORMS for v in ('', '_views')}
        for _ in range(args.rounds):
            for name in res:
                steps, n = _form(key, name.replace('_views', ''))
                stream = procedure.genFrameStream(steps, W, H, cb.DEPTH, timing=True, views=name.endswith('_views'))
                fps, stages = cb._leg(stream, noise[n], args.warmup)
                res[name]['edge'] = stream.edge
                stream.close()
                res[name]['fps'].append(fps)
                res[name]['stage_ms_per_frame'].append(stages)
                print('{} {}: {} fps, compute {} ms'.format(key, name, fps, stages['compute_ms']), file=sys.stderr, flush=True)
        for r in res.values():
            r['fps_median'] = median(r['fps'])
            for k in ('compute_ms', 'tobytes_ms', 'd2h_ms', 'h2d_ms', 'memcpy_ms'):
                r[k + '_median'] = median([s[k] for s in r['stage_ms_per_frame']])
        have, kept = res['rgb_rgb']['compute_ms_median'] - res['yuv_yuv']['compute_ms_median'], res['rgb_rgb']['compute_ms_median'] - res['yuv_rgb_net']['compute_ms_median']
        res['gate'] = {'planar_gain_ms': round(have, 3), 'rgb_out_gain_ms': round(kept, 3), 'share_kept': round(kept / have, 3) if have > 0 else None,
                       'holds': bool(have > 0 and kept >= 0.5 * have)}
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    cb._emit(result, args.out)


def summary(args):
    d = os.path.abspath(args.parent)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, g, o = load('kernel.json'), load('gain.json'), load('off.json')
    lines = ['# RGB frames from chains on 4:2:0 planes: measurements (`tools/planes_rgb_bench.py`)', '',
             'Everything below is written by `planes_rgb_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '',
             '## Kernel gate: `to_output_rgb420_kernel` beside `stitch_out_kernel<u16, 3, 4>`', '']
    if k:
        a, b = k['cases']['A_to_output_rgb420_kernel'], k['cases']['B_stitch_out_kernel']
        lines += ['MI355X, one device.  ' + k['frame'] + '; ' + k['timing'] + ', {} rounds of {} launches, the two legs alternating in one process.'.format(k['rounds'], k['reps']), '',
                  '| leg | median µs | fastest | spread over rounds | bytes moved | GB/s |', '|---|---|---|---|---|---|']
        for name, r in (('A `to_output_rgb420_kernel<u16, u16, 4>`', a), ('B `stitch_out_kernel<u16, 3, 4>` (a4 1080p -> 8K pool)', b)):
            lines.append('| {} | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['bytes'], r['GB_per_s']))
        lines += ['', 'Gate (A <= B + B\'s spread = {} µs): **{}**.'.format(a['bar_us'], 'holds' if a['holds'] else 'MISSED'), '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: the three forms', '']
    if g:
        lines += ['MI355X, one device; 1080p sources, ring depth {}, distinct noise frames.  One process, the configurations alternating {} times, {} timed frames per leg after {} '
                  'warm-up frames; medians over the legs, stage times in ms per frame.'.format(g['depth'], g['rounds'], g['frames'], g['warmup']), '',
                  '| stream | form | edge | fps (legs) | fps median | compute | tobytes | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|---|']
        for key, m in g['models'].items():
            for name, r in m.items():
                if name != 'gate':
                    lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r.get('edge'), r['fps'], r['fps_median'], r['compute_ms_median'],
                                                                                         r['tobytes_ms_median'], r['d2h_ms_median'], r['h2d_ms_median'], r['memcpy_ms_median']))
        lines.append('')
        for key, m in g['models'].items():
            t = m['gate']
            lines.append('{}: on the compute stage `yuv420p10le` -> `yuv420p10le` gains {} ms per frame over `bgr48le` -> `bgr48le`, `yuv420p10le` -> `bgr48le` {} ms: {} of it{}.'.format(
                key, t['planar_gain_ms'], t['rgb_out_gain_ms'], t['share_kept'],
                ' -- gate (at least half, on a4): **{}**'.format('holds' if t['holds'] else 'MISSED') if key == 'a4' else ''))
        lines.append('')
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
    lines += ['## Not measured here', '', 'The `bgr48le` -> `bgr48le` streams against the parent commit (only the planar streams run in `off`), `bench.py` (its figure is in the README), other sizes, 8-bit sinks, '
              '`reuse=True` with an RGB sink.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'gain', 'off', 'summary'])
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
    {'kernel': kernel, 'gain': gain, 'off': cb.off, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
