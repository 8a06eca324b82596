#!/usr/bin/env python
"""Frames per second of the video loop, streamed against serial, on seeded distinct 1080p 16-bit frames (measurement tool; results: profiles/frame_stream/summary.md).

    python tools/frame_stream_bench.py [--models a2,a4] [--frames 32] [--warmup 4] [--rounds 3] [--depths 2,3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o fs -f csv -- python tools/frame_stream_bench.py --kernels
    python tools/frame_stream_bench.py --kstats DIR/.../fs_kernel_stats.csv          (no device: reads that run's kernel stats)

serial   = procedure.runFrames over procedure.genProcess: blocking pageable upload, the chain, stitch -> fp32 copy -> quantise, blocking pageable download
streamed = procedure.runFramesStreamed over procedure.genFrameStream(depth): pinned ring, three queues, the stitch writing the samples itself

Both forms run in ONE process, alternating `rounds` times; a leg is `warmup` untimed frames, then `frames` frames between two host clock reads, the second one
behind a device synchronise.  The spread of the serial legs of one call is the noise floor the difference is held against.  The streamed legs also report the
ring's own per-stage times (host memcpy into the pinned buffer, H2D, compute, D2H from event timestamps, the host copy out of the pinned buffer).
a4 uses the synthetic weights of tests/golden_defs.py (as bench.py does); the frames are uniform noise -- every kernel's time is independent of the data.
--kernels: three serial and three streamed a4 frames and nothing else, for a kernel trace; --kstats prints, from that trace's kernel_stats.csv, stitch_out_kernel
against stitch8r + the fp32 copy + to_output3 on the 8K canvas and the bytes per second of each (the fused pass must move 4 B read + 2 B written per pixel-plane)."""
import argparse
import csv
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


def kstats(path):
    """average microseconds per call of the output edge's kernels in a rocprofv3 kernel_stats.csv of `--kernels` (a4: 3 x 4320 x 7680 pixel-planes, fp16 canvas, u16 out)"""
    planes = 3 * 4320 * 7680
    # bytes per pixel-plane each pass moves: pool fp32 -> canvas fp16; fp16 -> fp32; fp32 -> u16; pool fp32 -> u16
    passes = [('stitch8r_kernel', 6), ('float16tofloat32_copy_kernel', 6), ('to_output3_kernel', 6), ('stitch_out_kernel', 6)]
    rows = list(csv.DictReader(open(path)))
    out = {}
    for name, bpp in passes:
        hit = [r for r in rows if name in r['Name']]
        if not hit:
            out[name] = 'not measured'
            continue
        us = sum(float(r['TotalDurationNs']) for r in hit) / sum(int(r['Calls']) for r in hit) / 1e3
        out[name] = {'calls': sum(int(r['Calls']) for r in hit), 'avg_us': round(us, 1), 'bytes_per_pixel_plane': bpp, 'GB_per_s': round(planes * bpp / us / 1e3, 1)}
    three = [out[n] for n, _ in passes[:3]]
    if all(isinstance(v, dict) for v in three):
        out['three_passes'] = {'avg_us': round(sum(v['avg_us'] for v in three), 1), 'bytes_per_pixel_plane': 18}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='a2,a4')
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--depths', default='2,3')
    ap.add_argument('--out')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--kstats', metavar='CSV')
    args = ap.parse_args()
    if args.kstats:
        return kstats(args.kstats)

    import numpy as np
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, procedure, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file

    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_fs_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])

    if args.kernels:
        args.models, args.frames, args.warmup, args.rounds, args.depths = 'a4', 3, 0, 1, '2'
    n_all = args.warmup + args.frames
    rng = np.random.default_rng(2024)
    frames = [rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(n_all)]
    warm, timed = b''.join(frames[:args.warmup]), b''.join(frames[args.warmup:])
    del frames
    depths = [int(d) for d in args.depths.split(',')]
    sink = {'bytes': 0}

    def write(buf):
        sink['bytes'] += len(buf)

    def leg(run, data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(io.BytesIO(data).read)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == n, (got, n)
        return dt

    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'input': '{}x{} {}-bit noise, distinct frames'.format(W, H, BITS), 'models': {}}
    for key in args.models.split(','):
        scale = int(key[-1])
        steps = [{'op': 'buffer', 'bitDepth': BITS}, {'op': 'SR', 'model': key[:-1], 'scale': scale, 'ensemble': 0}]
        process, _ = procedure.genProcess(steps, bitDepth=BITS)
        serial = lambda read: procedure.runFrames(process, read, write, W, H, bitDepth=BITS)
        forms = [('serial', 0)] + [('streamed_depth{}'.format(d), d) for d in depths]
        res = {name: {'fps': [], 'ms_per_frame': []} for name, _ in forms}
        for _ in range(args.rounds):
            for name, depth in forms:
                # a ring lives for its own legs only: its pinned buffers (depth x 199 MB for an 8K frame) are not resident beside another form's
                stream = procedure.genFrameStream(steps, W, H, depth, timing=True) if depth else None
                run = serial if stream is None else (lambda read: procedure.runFramesStreamed(stream, read, write))
                if args.warmup:
                    leg(run, warm, args.warmup)
                if stream is not None:
                    for k in stream.backend.stats:
                        stream.backend.stats[k] = 0
                dt = leg(run, timed, args.frames)
                res[name]['fps'].append(round(args.frames / dt, 3))
                res[name]['ms_per_frame'].append(round(dt / args.frames * 1e3, 3))
                if stream is not None:
                    st = stream.backend.stats
                    res[name].setdefault('stage_ms_per_frame', []).append({k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'})
                    stream.close()
        for name in res:
            f = res[name]['fps']
            res[name]['fps_median'] = sorted(f)[len(f) // 2]
            res[name]['fps_spread'] = round(max(f) - min(f), 3)
        res['output'] = '{}x{} {}-bit, {:.1f} MB per frame'.format(W * scale, H * scale, BITS, W * scale * H * scale * 3 * 2 / 1e6)
        result['models'][key] = res
        print(json.dumps({key: res}), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(result, open(args.out, 'w'), indent=1)
    print(json.dumps(result))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
