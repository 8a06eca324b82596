#!/usr/bin/env python
"""Chains on the decoder's own Y'CbCr 4:2:0 planes against the RGB forms they stand beside (measurement tool; results: profiles/planes/summary.md,
profiles/planes/planes_bench.json).  Needs a GPU.

    python tools/planes_bench.py [--rounds 5] [--reps 50] [--frames 24] [--warmup 4] [--stream-rounds 2] [--depths 2,3] [--no-stream] [--out FILE.json]

kernel   One process, `rounds` alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/yuv_bench.py).
         gate    the 8K Y plane (plan (1, 1080, 1920), x4, tiles of 256, fp16 canvas rounding): stitch_planes_kernel at C = 1, depth 16 writes the bytes of
                 moe_stitch_out(C = 1, bits = 16); it holds when its median is no more than that kernel's median plus that kernel's own round-to-round spread.
         record  depth 10 on the same plane and the C = 2 chroma plan (2, 540, 960), each beside the two passes it replaces (moe_stitch to an fp16 canvas, then
                 moe_to_output); to_float_planes_kernel on a 1080p frame in GB/s.
stream   a4, 1080p -> 8K: yuv420p10le in and out against the best RGB form (bgr48le in, yuv420p10le out), alternating in one process: frames per second, the
         ring's per-stage times, and the ratio of the plane-tile pixels the two forms send through the net, from their plans.  A record, not a gate."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W, CROP, FMT = 1080, 1920, 256, 'yuv420p10le'


def median(v):
    return sorted(v)[len(v) // 2]


def plan_for(shape):
    from moephoto_amd.imageProcess import TilePlan
    return TilePlan(shape, 1 << 40, 1e-3, 5, 4, 8, CROP)


def kernels(args, torch):
    from moephoto_amd import _lib, pixfmt
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream

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

    cases, moved, keep = {}, {}, []
    for name, shape in (('y', (1, H, W)), ('c', (2, H // 2, W // 2))):
        C = shape[0]
        pl = plan_for(shape)
        px = C * pl.outH * pl.outW
        pool = torch.rand(pl.pool_elems(C), dtype=torch.float32, device=dev)
        out = torch.empty((px,), dtype=torch.int16, device=dev)
        canvas = torch.empty((C, pl.outH, pl.outW), dtype=torch.float16, device=dev)
        keep += [pl, pool, out, canvas]

        def planes(depth, pl=pl, pool=pool, out=out, C=C):
            return lambda: _lib.check(L.moe_stitch_planes(pl._h, 0, pool.data_ptr(), None, C, _lib.F16, depth, out.data_ptr(), st))

        def two_passes(depth, pl=pl, pool=pool, out=out, canvas=canvas, C=C):
            def f():
                _lib.check(L.moe_stitch(pl._h, 0, pool.data_ptr(), None, C, canvas.data_ptr(), _lib.F16, st))
                _lib.check(L.moe_to_output(canvas.data_ptr(), _lib.F16, C * pl.outH, pl.outW, 1, depth, out.data_ptr(), _lib.U16, 0, st))
            return f
        if name == 'y':
            cases['y_stitch_out_c1_16'] = lambda pl=pl, pool=pool, out=out: _lib.check(L.moe_stitch_out(pl._h, 0, pool.data_ptr(), None, 1, _lib.F16, 16, out.data_ptr(), _lib.U16, st))
            cases['y_stitch_planes_16'] = planes(16)
            moved['y_stitch_out_c1_16'] = moved['y_stitch_planes_16'] = px * (4 + 2)
        cases[name + '_stitch_planes_10'] = planes(10)
        cases[name + '_stitch_then_to_output_10'] = two_passes(10)
        moved[name + '_stitch_planes_10'] = px * (4 + 2)
        moved[name + '_stitch_then_to_output_10'] = px * (4 + 2 + 2 + 2)
    n = pixfmt.frameBytes(FMT, W, H)
    raw = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
    y, c = torch.empty((1, H, W), dtype=torch.float16, device=dev), torch.empty((2, H // 2, W // 2), dtype=torch.float16, device=dev)
    cases['to_float_planes_1080p_10'] = lambda: _lib.check(L.moe_planes_to_float(raw.data_ptr(), 10, H, W, y.data_ptr(), c.data_ptr(), _lib.F16, 0, st))
    moved['to_float_planes_1080p_10'] = n + n
    rounds = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, f in cases.items():
            rounds[k].append(device_us(f))
    res = {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2), 'bytes': moved[k],
               'GB_per_s': round(moved[k] / median(v) / 1e3, 1)} for k, v in rounds.items()}
    base, new = res['y_stitch_out_c1_16'], res['y_stitch_planes_16']
    new['bar_us'] = round(base['median_us'] + base['spread_us'], 2)
    new['holds'] = new['median_us'] <= new['bar_us']
    del keep, raw, y, c
    torch.cuda.empty_cache()
    return {'planes': 'Y: 1 x {} x {}, chroma: 2 x {} x {}, from 1080p x4 plans, tiles of {}'.format(4 * H, 4 * W, 2 * H, 2 * W, CROP), 'reps': args.reps, 'cases': res}


def tile_pixels(shape):
    """Plane-pixels a plan sends through the net: the sum over its tiles of planes x tile height x tile width."""
    pl = plan_for(shape)
    return shape[0] * sum((t[1] - t[0]) * (t[3] - t[2]) for t in pl.tiles)


def stream(args, torch):
    import numpy as np
    import golden_defs as gd
    from moephoto_amd import pixfmt, procedure, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_planes_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    rng = np.random.default_rng(2024)
    total = args.warmup + args.frames
    data = {'bgr48le': [rng.integers(0, 1 << 16, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(total)],
            FMT: [rng.integers(0, 1 << 10, pixfmt.frameBytes(FMT, W, H) // 2, dtype=np.uint16).tobytes() for _ in range(total)]}
    data = {k: (b''.join(v[:args.warmup]), b''.join(v[args.warmup:])) for k, v in data.items()}
    sink = {'bytes': 0}

    def write(buf):
        sink['bytes'] += len(buf)

    def leg(s, raw, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(s, io.BytesIO(raw).read, write)
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0

    sr = {'op': 'SR', 'model': 'a', 'scale': 4, 'ensemble': 0}
    steps = {'bgr48le': [{'op': 'buffer', 'bitDepth': 16}, sr, {'op': 'output', 'pixFmt': FMT}], FMT: [{'op': 'buffer', 'pixFmt': FMT}, sr]}
    forms = [(src, d) for d in [int(v) for v in args.depths.split(',')] for src in ('bgr48le', FMT)]
    res = {'{}_in_depth{}'.format(src, d): {'fps': [], 'stage_ms_per_frame': []} for src, d in forms}
    for _ in range(args.stream_rounds):
        for src, d in forms:
            s = procedure.genFrameStream(steps[src], W, H, d, timing=True)          # (a ring lives for its own legs only)
            warm, timed = data[src]
            if args.warmup:
                leg(s, warm, args.warmup)
            for k in s.backend.stats:
                s.backend.stats[k] = 0
            sink['bytes'] = 0
            dt = leg(s, timed, args.frames)
            r = res['{}_in_depth{}'.format(src, d)]
            r['edge'] = s.edge
            r['fps'].append(round(args.frames / dt, 3))
            st = s.backend.stats
            r['stage_ms_per_frame'].append({k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'})
            r['MB_in_per_frame'], r['MB_out_per_frame'] = round(len(timed) / args.frames / 1e6, 1), round(sink['bytes'] / args.frames / 1e6, 1)
            s.close()
    for r in res.values():
        r['fps_median'] = median(r['fps'])
    shutil.rmtree(tmp, ignore_errors=True)
    planar, rgb = tile_pixels((1, H, W)) + tile_pixels((2, H // 2, W // 2)), tile_pixels((3, H, W))
    return {'input': '{}x{} noise, distinct frames; a4 (synthetic weights) -> {}x{}; output {} in both forms'.format(W, H, 4 * W, 4 * H, FMT), 'frames': args.frames,
            'warmup': args.warmup, 'rounds': args.stream_rounds, 'forms': res,
            'plane_tile_pixels': {'planar': planar, 'rgb': rgb, 'ratio': round(planar / rgb, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--stream-rounds', type=int, default=2)
    ap.add_argument('--depths', default='2,3')
    ap.add_argument('--no-stream', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from moephoto_amd import _lib
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    result = {'kernel': kernels(args, torch)}
    print(json.dumps(result), flush=True)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(result, open(args.out, 'w'), indent=1)
    save()
    if not args.no_stream:
        result['stream'] = stream(args, torch)
        print(json.dumps({'stream': result['stream']}), flush=True)
        save()
    return 0 if result['kernel']['cases']['y_stitch_planes_16']['holds'] else 1


if __name__ == '__main__':
    sys.exit(main())
