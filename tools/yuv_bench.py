#!/usr/bin/env python
"""The Y'CbCr 4:2:0 output edge against the interleaved one it stands beside (measurement tool; results: profiles/yuv/summary.md, profiles/yuv/yuv_bench.json).

    python tools/yuv_bench.py [--rounds 5] [--reps 50] [--frames 24] [--warmup 4] [--stream-rounds 2] [--depths 2,3] [--no-stream] [--out FILE.json]

kernel   stitch_yuv_kernel (u16, depth 10) and stitch_out_kernel<u16, 3, 4> on the SAME 8K pool (3 x 4320 x 7680, x4 of 1080p, tiles of 256) in one process, `rounds`
         alternating rounds of `reps` back-to-back launches between device events, microseconds per launch (as tools/stitch_bench.py).  The YUV edge reads the same
         pool and writes half the bytes; it holds when its median is no more than stitch_out's median plus stitch_out's own round-to-round spread (max - min).
         Also timed, for the record: the u8 form and the unfused moe_to_yuv beside moe_to_output on the fp16 8K canvas.
stream   a4, 1080p -> 8K, 16-bit input: genFrameStream with {'op': 'output', 'pixFmt': 'yuv420p10le'} against today's bgr48le, alternating in one process
         (as tools/frame_stream_bench.py): frames per second and the ring's per-stage times.  A record, not a gate: the host side of the box decides it."""
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

H, W, BITS, CROP = 1080, 1920, 16, 256


def median(v):
    return sorted(v)[len(v) // 2]


def kernels(args, torch):
    from moephoto_amd import _lib, pixfmt
    from moephoto_amd.imageProcess import TilePlan
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

    pl = TilePlan((3, H, W), 1 << 40, 1e-3, 5, 4, 8, CROP)
    pool = torch.rand(pl.pool_elems(3), dtype=torch.float32, device=dev)
    samples = torch.empty((pl.outH, pl.outW, 3), dtype=torch.int16, device=dev)
    frame10 = torch.empty((pixfmt.frameBytes('yuv420p10le', pl.outW, pl.outH),), dtype=torch.uint8, device=dev)
    frame8 = torch.empty((pixfmt.frameBytes('yuv420p', pl.outW, pl.outH),), dtype=torch.uint8, device=dev)
    canvas = torch.rand((3, pl.outH, pl.outW), dtype=torch.float32, device=dev).half()
    cases = {
        'stitch_out_u16': lambda: _lib.check(L.moe_stitch_out(pl._h, 0, pool.data_ptr(), None, 3, _lib.F16, 16, samples.data_ptr(), _lib.U16, st)),
        'stitch_yuv_u16_d10': lambda: _lib.check(L.moe_stitch_yuv(pl._h, 0, pool.data_ptr(), None, _lib.F16, 10, 0, 0, frame10.data_ptr(), st)),
        'stitch_yuv_u8': lambda: _lib.check(L.moe_stitch_yuv(pl._h, 0, pool.data_ptr(), None, _lib.F16, 8, 0, 0, frame8.data_ptr(), st)),
        'to_output_u16': lambda: _lib.check(L.moe_to_output(canvas.data_ptr(), _lib.F16, pl.outH, pl.outW, 3, 16, samples.data_ptr(), _lib.U16, 0, st)),
        'to_yuv_u16_d10': lambda: _lib.check(L.moe_to_yuv(canvas.data_ptr(), _lib.F16, pl.outH, pl.outW, 10, 0, 0, frame10.data_ptr(), 0, st)),
    }
    rounds = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, f in cases.items():
            rounds[k].append(device_us(f))
    px = pl.outH * pl.outW
    moved = {'stitch_out_u16': px * 3 * (4 + 2), 'stitch_yuv_u16_d10': px * 3 * 4 + px * 3, 'stitch_yuv_u8': px * 3 * 4 + px * 3 // 2,
             'to_output_u16': px * 3 * (2 + 2), 'to_yuv_u16_d10': px * 3 * 2 + px * 3}
    res = {k: {'rounds_us': v, 'median_us': median(v), 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2), 'bytes': moved[k],
               'GB_per_s': round(moved[k] / median(v) / 1e3, 1)} for k, v in rounds.items()}
    base, new = res['stitch_out_u16'], res['stitch_yuv_u16_d10']
    new['bar_us'] = round(base['median_us'] + base['spread_us'], 2)
    new['holds'] = new['median_us'] <= new['bar_us']
    del pool, samples, frame10, frame8, canvas
    torch.cuda.empty_cache()
    return {'canvas': '3 x {} x {} from a 1080p x4 plan, tiles of {}'.format(pl.outH, pl.outW, CROP), 'reps': args.reps, 'cases': res}


def stream(args, torch):
    import numpy as np
    import golden_defs as gd
    from moephoto_amd import procedure, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_yuv_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    rng = np.random.default_rng(2024)
    frames = [rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(args.warmup + args.frames)]
    warm, timed = b''.join(frames[:args.warmup]), b''.join(frames[args.warmup:])
    del frames
    sink = {'bytes': 0}

    def write(buf):
        sink['bytes'] += len(buf)

    def leg(s, data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(s, io.BytesIO(data).read, write)
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0

    base = [{'op': 'buffer', 'bitDepth': BITS}, {'op': 'SR', 'model': 'a', 'scale': 4, 'ensemble': 0}]
    forms = [(fmt, d, base + ([{'op': 'output', 'pixFmt': fmt}] if fmt != 'bgr48le' else [])) for d in [int(v) for v in args.depths.split(',')] for fmt in ('bgr48le', 'yuv420p10le')]
    res = {'{}_depth{}'.format(fmt, d): {'fps': [], 'stage_ms_per_frame': []} for fmt, d, _ in forms}
    for _ in range(args.stream_rounds):
        for fmt, d, steps in forms:
            s = procedure.genFrameStream(steps, W, H, d, timing=True)          # (a ring lives for its own legs only: depth x 199 MB of pinned memory)
            if args.warmup:
                leg(s, warm, args.warmup)
            for k in s.backend.stats:
                s.backend.stats[k] = 0
            sink['bytes'] = 0
            dt = leg(s, timed, args.frames)
            r = res['{}_depth{}'.format(fmt, d)]
            r['fps'].append(round(args.frames / dt, 3))
            st = s.backend.stats
            r['stage_ms_per_frame'].append({k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'})
            r['MB_per_frame'] = round(sink['bytes'] / args.frames / 1e6, 1)
            s.close()
    for r in res.values():
        r['fps_median'] = median(r['fps'])
    shutil.rmtree(tmp, ignore_errors=True)
    return {'input': '{}x{} {}-bit noise, distinct frames; a4 (synthetic weights) -> {}x{}'.format(W, H, BITS, 4 * W, 4 * H), 'frames': args.frames, 'warmup': args.warmup,
            'rounds': args.stream_rounds, 'forms': res}


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


if __name__ == '__main__':
    main()
