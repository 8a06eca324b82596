#!/usr/bin/env python
"""The 3D LUT colour step (measurement tool; results: profiles/lut3d/summary.md and the JSON files beside it).  Needs a GPU.

    python tools/lut3d_bench.py kernel  [--rounds 7] [--reps 50] [--out FILE.json]
    python tools/lut3d_bench.py streams [--models a4,a2] [--frames 24] [--warmup 4] [--rounds 3] [--out FILE.json]
    python tools/lut3d_bench.py off PARENT_TREE [--models ..] [--frames ..] [--rounds 3] [--limit 300] [--out FILE.json]
    python tools/lut3d_bench.py summary DIR          (DIR holds kernel.json / streams.json / off.json: whichever exist are written up as DIR/summary.md)

kernel   one process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/planes_rgb_bench.py):
         A = to_output_lut3d_kernel<u16, u16> on an 8K bgr48le frame -> bgr48le, d = 33, non-uniform vertices, a smooth frame (ramps plus low noise);
         B = to_output_rgb420_kernel<u16, u16, 4> on an 8K yuv420p16le frame -> bgr48le, the project's closest edge, which writes the same 199 MB.
         Gate: A's median <= 1.5 x B's median.  Reported without a gate, in the same rounds: A on uniform-noise frames (worst table locality), d = 17 and d = 65
         (smooth and noise), and 8-bit sinks.
streams  the 1080p bgr48le streams of a4 (-> 8K) and a2 (-> 4K), ring depth 2, with and without a 'lut' step (d = 33, non-uniform), alternating `rounds` times in
         one process: frames per second and the ring's per-stage times.  Gate: the compute stage's increase <= 2 x the kernel's own time on a frame of that size
         (measured here, on the stream's own output size, between device events).
off      the same streams WITHOUT the step in PARENT_TREE (a checkout of the parent commit with its library built) and in this tree, as alternating child processes;
         this tree must be within the parent's own spread.

a4 uses the synthetic weights of tests/golden_defs.py (as bench.py does); the a4 / a2 kernels' time is independent of the data, the LUT kernel's is not: its frames
are named above."""
import argparse
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
import chroma_bench as cb          # noqa: E402  (the stream leg, the set-up and the emit helper are that tool's)

median, H, W = cb.median, cb.H, cb.W
GATE_KERNEL, GATE_STREAM = 1.5, 2.0


def _lut(d, uniform=False):
    import numpy as np
    from moephoto_amd import lut3d
    rng = np.random.default_rng(d)
    table = (lut3d.identity(d) + (rng.random((3, d, d, d), np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)          # a look: the identity, bent
    if uniform:
        return table, lut3d.uniform(d)
    v = lut3d.uniform(d).astype(np.float64) ** 1.6          # non-uniform vertices: dense in the shadows
    return table, np.ascontiguousarray(v.astype(np.float32))


def _frame16(kind, h, w, dev):
    """An h x w x 3 frame of 16-bit samples on the device: 'smooth' -- a horizontal, a vertical and a diagonal ramp plus noise of 1 % of full scale; 'noise' -- uniform
    noise over all 16 bits (no two neighbouring pixels share a cell: the worst table locality)."""
    import torch
    if kind == 'noise':
        return torch.randint(-32768, 32767, (h, w, 3), dtype=torch.int16, device=dev)
    y, x = torch.arange(h, device=dev, dtype=torch.float32)[:, None] / h, torch.arange(w, device=dev, dtype=torch.float32)[None, :] / w
    ramps = torch.stack([x.expand(h, w), y.expand(h, w), ((x + y) / 2).expand(h, w)], 2)
    v = (ramps * 0.98 + torch.rand((h, w, 3), device=dev) * 0.01).clamp(0, 1) * 65535
    return (v.to(torch.int32) - 65536 * (v >= 32768).to(torch.int32)).to(torch.int16)          # (uint16 samples in int16 storage)


def _device_us(f, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def kernel(args):
    cb._path(HERE)
    import ctypes
    import torch
    from moephoto_amd import _lib, pixfmt
    from moephoto_amd.imageProcess import _LutHandle
    _lib.require_device()
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    oh, ow = 4 * H, 4 * W
    frames = {k: _frame16(k, oh, ow, dev) for k in ('smooth', 'noise')}
    out16, out8 = torch.empty((oh, ow, 3), dtype=torch.int16, device=dev), torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
    handles = {d: _LutHandle(*_lut(d), 0) for d in (17, 33, 65)}
    (ox, cx) = pixfmt.chromaTable('bicubic', 2, 'center')
    flat = [c for r in cx for c in r]
    tabs = ((ctypes.c_int16 * 8)(*flat), (ctypes.c_int8 * 2)(*ox), (ctypes.c_int32 * 5)(*pixfmt.rgbCoefficients('bt709', 16, 16)))
    planar = torch.randint(-32768, 32767, (oh * ow * 3 // 2,), dtype=torch.int16, device=dev)

    def lut(d, kind, bits=16):
        out = out16 if bits == 16 else out8
        return lambda: _lib.check(L.moe_lut3d_run(handles[d]._h, frames[kind].data_ptr(), 16, oh, ow, out.data_ptr(), bits, 0, 1.0, st))
    cases = {'A_lut3d_d33_smooth': lut(33, 'smooth'),
             'B_to_output_rgb420_kernel': lambda: _lib.check(L.moe_planes_to_rgb(planar.data_ptr(), 16, oh, ow, out16.data_ptr(), 16, 0, 0, 4, tabs[0], tabs[1], tabs[0], tabs[1], tabs[2], 0, st)),
             'lut3d_d33_noise': lut(33, 'noise'), 'lut3d_d17_smooth': lut(17, 'smooth'), 'lut3d_d17_noise': lut(17, 'noise'),
             'lut3d_d65_smooth': lut(65, 'smooth'), 'lut3d_d65_noise': lut(65, 'noise'), 'lut3d_d33_smooth_8bit_sink': lut(33, 'smooth', 8), 'lut3d_d33_noise_8bit_sink': lut(33, 'noise', 8)}
    px = oh * ow
    moved = {k: 6 * px + (3 * px if k.endswith('8bit_sink') else 6 * px) for k in cases}
    moved['B_to_output_rgb420_kernel'] = 2 * (px * 3 // 2) + 6 * px
    rounds = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, f in cases.items():
            rounds[k].append(_device_us(f, args.reps))
    res = {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2), 'frame_bytes': moved[k],
               'GB_per_s': round(moved[k] / median(v) / 1e3, 1)} for k, v in rounds.items()}
    a, b = res['A_lut3d_d33_smooth'], res['B_to_output_rgb420_kernel']
    a['bar_us'] = round(GATE_KERNEL * b['median_us'], 2)
    a['ratio'] = round(a['median_us'] / b['median_us'], 3)
    a['holds'] = a['median_us'] <= a['bar_us']
    cb._emit({'frame': '{} x {} bgr48le -> bgr48le'.format(ow, oh), 'reps': args.reps, 'rounds': args.rounds, 'timing': 'device events around `reps` back-to-back launches',
              'table_bytes': {str(d): 16 * d ** 3 for d in handles}, 'cases': res}, args.out)


def _steps(key, lut):
    steps = [{'op': 'buffer', 'bitDepth': 16}, {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}]
    if lut:
        table, vertices = _lut(33)
        steps.append({'op': 'lut', 'table': table, 'vertices': vertices})
    return steps


def _noise_frames(n):
    import numpy as np
    rng = np.random.default_rng(2024)
    return [rng.integers(0, 1 << 16, W * H * 3, dtype=np.uint16).tobytes() for _ in range(n)]


def _legs(procedure, key, forms, frames, args):
    res = {name: {'fps': [], 'stage_ms_per_frame': []} for name in forms}
    for _ in range(args.rounds):
        for name in forms:
            stream = procedure.genFrameStream(_steps(key, name == 'lut'), W, H, cb.DEPTH, timing=True)
            fps, stages = cb._leg(stream, frames, args.warmup)
            res[name]['edge'] = stream.edge
            stream.close()
            res[name]['fps'].append(fps)
            res[name]['stage_ms_per_frame'].append(stages)
            print('{} {}: {} fps, compute {} ms'.format(key, name, fps, stages['compute_ms']), file=sys.stderr, flush=True)
    for r in res.values():
        r['fps_median'] = median(r['fps'])
        for k in ('compute_ms', 'tobytes_ms', 'd2h_ms', 'h2d_ms', 'memcpy_ms'):
            r[k + '_median'] = median([s[k] for s in r['stage_ms_per_frame']])
    return res


def streams(args):
    tmp = cb._setup(HERE)
    import torch
    from moephoto_amd import _lib, procedure
    from moephoto_amd.imageProcess import _LutHandle
    frames = _noise_frames(args.warmup + args.frames)
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'models': {}}
    L, dev, handle = _lib.lib(), torch.device('cuda:0'), _LutHandle(*_lut(33), 0)
    for key in args.models.split(','):
        res = _legs(procedure, key, ('plain', 'lut'), frames, args)
        s = int(key[-1])
        # the kernel's own time on this stream's output size, on what the stream hands it: an upscaled noise frame is smooth at the table's scale; both kinds are timed
        oh, ow = s * H, s * W
        out = torch.empty((oh, ow, 3), dtype=torch.int16, device=dev)
        own = {}
        for kind in ('smooth', 'noise'):
            src = _frame16(kind, oh, ow, dev)
            f = lambda: _lib.check(L.moe_lut3d_run(handle._h, src.data_ptr(), 16, oh, ow, out.data_ptr(), 16, 0, 1.0, torch.cuda.current_stream().cuda_stream))
            own[kind] = median([_device_us(f, 20) for _ in range(5)])
        inc = round(res['lut']['compute_ms_median'] - res['plain']['compute_ms_median'], 3)
        res['gate'] = {'kernel_us': own, 'compute_increase_ms': inc, 'bar_ms': round(GATE_STREAM * own['smooth'] / 1e3, 3), 'holds': bool(inc <= GATE_STREAM * own['smooth'] / 1e3)}
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    cb._emit(result, args.out)


def cost(args):
    """One child of `off`: the streams without the step, in the tree at --root."""
    root = os.path.abspath(args.root or HERE)
    tmp = cb._setup(root)
    from moephoto_amd import procedure
    frames = _noise_frames(args.warmup + args.frames)
    result = {'root': root, 'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'models': {}}
    for key in args.models.split(','):
        result['models'][key] = _legs(procedure, key, ('plain',), frames, args)['plain']
    shutil.rmtree(tmp, ignore_errors=True)
    cb._emit(result, args.out)


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
                sys.exit('lut3d_bench off: the {} child of round {} ended with status {}; nothing more is started'.format(name, r, p.returncode))
            legs.append((name, json.loads(p.stdout.strip().splitlines()[-1])))
    out = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': cb.DEPTH, 'order': [n for n, _ in legs], 'models': {}}
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
    cb._emit(out, args.out)


def summary(args):
    d = os.path.abspath(args.parent)
    load = lambda name: json.load(open(os.path.join(d, name))) if os.path.exists(os.path.join(d, name)) else None
    k, s, o = load('kernel.json'), load('streams.json'), load('off.json')
    word = lambda ok: 'held' if ok else 'MISSED'
    lines = ['# The 3D LUT colour step: measurements (`tools/lut3d_bench.py`)', '',
             'Everything below is written by `lut3d_bench.py summary` from the JSON files in this directory; a part whose file is missing was not measured.', '',
             '## Kernel: `to_output_lut3d_kernel<u16, u16>` beside `to_output_rgb420_kernel<u16, u16, 4>`', '']
    if k:
        c = k['cases']
        a, b = c['A_lut3d_d33_smooth'], c['B_to_output_rgb420_kernel']
        lines += ['MI355X, one device.  ' + k['frame'] + '; ' + k['timing'] + ', {} rounds of {} launches, all legs alternating in one process.  The device\'s table: {}.'.format(
                      k['rounds'], k['reps'], ', '.join('d = {}: {} bytes'.format(dd, n) for dd, n in sorted(k['table_bytes'].items(), key=lambda t: int(t[0])))), '',
                  '| leg | median µs | fastest | spread over rounds | frame bytes moved | GB/s |', '|---|---|---|---|---|---|']
        for name, r in c.items():
            lines.append('| `{}` | {} | {} | {} | {} | {} |'.format(name, r['median_us'], r['fastest_us'], r['spread_us'], r['frame_bytes'], r['GB_per_s']))
        lines += ['', 'Kernel gate (d = 33, non-uniform vertices, smooth frame: A <= {} x B = {} µs): A / B = {}: **{}**.'.format(GATE_KERNEL, a['bar_us'], a['ratio'], word(a['holds'])),
                  '', 'Without a gate: uniform-noise frames, d = 17, d = 65 (its table does not fit one XCD\'s L2) and 8-bit sinks are the other rows of the table.', '']
    else:
        lines += ['Not measured.', '']
    lines += ['## Streams: with and without the step', '']
    if s:
        lines += ['MI355X, one device; 1080p `bgr48le` sources, ring depth {}, distinct noise frames.  One process, the two forms alternating {} times, {} timed frames per leg after {} '
                  'warm-up frames; medians over the legs, stage times in ms per frame.'.format(s['depth'], s['rounds'], s['frames'], s['warmup']), '',
                  '| stream | form | edge | fps (legs) | fps median | compute | tobytes | d2h | h2d | memcpy |', '|---|---|---|---|---|---|---|---|---|---|']
        for key, m in s['models'].items():
            for name, r in m.items():
                if name != 'gate':
                    lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, name, r.get('edge'), r['fps'], r['fps_median'], r['compute_ms_median'],
                                                                                         r['tobytes_ms_median'], r['d2h_ms_median'], r['h2d_ms_median'], r['memcpy_ms_median']))
        lines.append('')
        for key, m in s['models'].items():
            t = m['gate']
            lines.append('{}: the compute stage grows by {} ms per frame; the kernel alone on a frame of the stream\'s output size takes {} µs (smooth) / {} µs (noise).  Stream gate '
                         '(increase <= {} x the kernel\'s time = {} ms): **{}**.'.format(key, t['compute_increase_ms'], t['kernel_us']['smooth'], t['kernel_us']['noise'], GATE_STREAM, t['bar_ms'], word(t['holds'])))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    lines += ['## No cost when off: the streams without the step, against the parent commit', '']
    if o:
        lines += ['Alternating child processes ({}), {} timed frames per leg after {} warm-up frames.'.format(', '.join(o['order']), o['frames'], o['warmup']), '',
                  '| stream | parent fps (legs) | median | tree fps (legs) | median | parent\'s spread | tree - parent | within |', '|---|---|---|---|---|---|---|---|']
        for key, m in o['models'].items():
            lines.append('| {} | {} | {} | {} | {} | {} | {} | {} |'.format(key, m['parent']['fps'], m['parent']['fps_median'], m['tree']['fps'], m['tree']['fps_median'],
                                                                         m['parent_spread']['fps'], m['tree_against_parent']['fps'], 'held' if m['holds'] else 'MISSED'))
        lines.append('')
    else:
        lines += ['Not measured.', '']
    extra = os.path.join(d, 'not_measured.md')
    lines += ['## Not measured here', '', open(extra).read().strip() if os.path.exists(extra) else
              'Planar sources with an RGB `pixFmt` in front of the step, `reuse=True`, 8-bit sources, strengths other than 1, `genProcess` on still images.', '']
    open(os.path.join(d, 'summary.md'), 'w').write('\n'.join(lines))
    print(os.path.join(d, 'summary.md'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'streams', 'off', 'cost', 'summary'])
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
        args.rounds = 7 if args.mode == 'kernel' else 3
    {'kernel': kernel, 'streams': streams, 'off': off, 'cost': cost, 'summary': summary}[args.mode](args)


if __name__ == '__main__':
    main()
