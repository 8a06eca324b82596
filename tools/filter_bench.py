#!/usr/bin/env python
"""What the DN step's fused edge (moe_stitch_mix / moe_run_plan_filter) costs and saves on a 1080p frame (measurement tool; results: profiles/filter/summary.md).

    python tools/filter_bench.py [--reps 20] [--rounds 5] [--frames 16] [--out FILE.json]

One process, dn_lite5, strength 0.6, 3 planes, fp16, tiles of 256; every comparison alternates its two sides `rounds` times and reports the fastest and the spread.

kernels   device time between two events around `reps` back-to-back repetitions, per repetition, on one pool of tile results (moe_run_plan_ex, do_stitch = 0):
            canvas form   moe_stitch_mix(bits 0)    against  moe_stitch (stitch8r) + torch's  s * c, (1 - s) * inp, +  (three elementwise kernels)
            sample form   moe_stitch_mix(bits 16)   against  the same + the fp32 copy (toFloat) + moe_to_output (to_output3)
frame     imageProcess._RGBFilter on a resident frame, host clock around `frames` calls behind a device synchronise, config.filterOnDevice on against off
memory    torch's peak allocation during one _RGBFilter call above what was allocated before it (the engine's own pools are hipMalloc'ed and the same on both sides)
stream    frames per second of [buffer 16, DN lite5 0.6] through genFrameStream (depth 2) with the flag on ('filter' edge) and off ('quantise' edge), and serial"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W, BITS, CROP, STRENGTH = 1080, 1920, 16, 256, 0.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--out')
    args = ap.parse_args()

    import numpy as np
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, imageProcess as ip, procedure, runDN
    from moephoto_amd.config import config

    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_dn = gd.ZOO, 0, True, CROP
    dev = torch.device('cuda:0')
    L = _lib.lib()
    opt = runDN.getOpt({'op': 'DN', 'model': 'lite5', 'strength': STRENGTH})
    x = torch.from_numpy(np.random.default_rng(7).random((3, H, W), dtype=np.float32)).to(dev).half()
    ip.doCrop(opt, x)                                      # finalizes the net on the device, plans the shape
    plan = ip._plan_for(opt, x.shape)
    xp = plan.padImage(x)
    st = torch.cuda.current_stream().cuda_stream
    pool = torch.empty(plan.pool_elems(3), dtype=torch.float32, device=dev)
    sC, sH, sW = xp.stride()
    _lib.check(L.moe_run_plan_ex(opt.modelCached._h, plan._h, xp.data_ptr(), _lib.F16, sC, sH, sW, None, _lib.F16, 0, pool.data_ptr(), 0, 1, 0, st))
    canvas = torch.empty((3, plan.outH, plan.outW), dtype=torch.float16, device=dev)
    mixed = torch.empty_like(canvas)
    q_ref = torch.empty((plan.outH, plan.outW, 3), dtype=torch.int16, device=dev)
    q_mix = torch.empty_like(q_ref)
    s = STRENGTH
    tile_off = torch.tensor(plan.tile_offsets(3), dtype=torch.int64, device=dev)

    def passes(sample):
        _lib.check(L.moe_stitch_dev(plan._h, 0, pool.data_ptr(), tile_off.data_ptr(), 3, canvas.data_ptr(), _lib.F16, st))
        y = s * canvas + (1 - s) * xp[:, :plan.outH, :plan.outW]
        if sample:
            f = y.float()
            _lib.check(L.moe_to_output(f.data_ptr(), _lib.F32, plan.outH, plan.outW, 3, BITS, q_ref.data_ptr(), _lib.U16, 0, st))
        return y

    def fused(sample):
        dst = q_mix if sample else mixed
        _lib.check(L.moe_stitch_mix(plan._h, 0, pool.data_ptr(), None, 3, xp.data_ptr(), _lib.F16, sC, sH, sW, None, 0, 0, s, BITS if sample else 0,
                                    dst.data_ptr(), _lib.U16 if sample else _lib.F16, st))

    y = passes(True)
    fused(False)
    fused(True)
    torch.cuda.synchronize()
    assert torch.equal(y, mixed) and torch.equal(q_ref, q_mix), 'the two forms disagree'

    def device_us(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        f()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    result = {'frame': '{} x {} x 3 fp16, dn_lite5, strength {}, tiles of {}: {} tiles'.format(W, H, STRENGTH, CROP, plan.n_tiles), 'reps': args.reps, 'rounds': args.rounds}
    kern = {}
    for name, sample in (('canvas', False), ('sample', True)):
        a, b = [], []
        for _ in range(args.rounds):
            a.append(device_us(lambda: passes(sample)))
            b.append(device_us(lambda: fused(sample)))
        kern[name] = {'passes_us': [round(v, 1) for v in a], 'fused_us': [round(v, 1) for v in b], 'passes_fastest_us': round(min(a), 1), 'fused_fastest_us': round(min(b), 1)}
    # the stitch alone, for the bytes per second of the fused pass next to it
    only = [device_us(lambda: _lib.check(L.moe_stitch_dev(plan._h, 0, pool.data_ptr(), tile_off.data_ptr(), 3, canvas.data_ptr(), _lib.F16, st))) for _ in range(args.rounds)]
    kern['stitch8r_alone_fastest_us'] = round(min(only), 1)
    px = 3 * plan.outH * plan.outW
    kern['fused_canvas_GB_per_s'] = round(px * (4 + 2 + 2) / kern['canvas']['fused_fastest_us'] / 1e3, 1)       # pool fp32 + inp fp16 read, canvas fp16 written
    kern['fused_sample_GB_per_s'] = round(px * (4 + 2 + 2) / kern['sample']['fused_fastest_us'] / 1e3, 1)       # ... u16 written
    result['kernels'] = kern
    print(json.dumps({'kernels': kern}), flush=True)

    def frame_ms(flag):
        config.filterOnDevice = flag
        ip._RGBFilter(opt, x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.frames):
            ip._RGBFilter(opt, x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.frames * 1e3

    def peak_bytes(flag):
        config.filterOnDevice = flag
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        y = ip._RGBFilter(opt, x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        del y
        return peak

    try:
        on, off = [], []
        for _ in range(args.rounds):
            off.append(frame_ms(False))
            on.append(frame_ms(True))
        result['frame_ms'] = {'off': [round(v, 3) for v in off], 'on': [round(v, 3) for v in on], 'off_fastest': round(min(off), 3), 'on_fastest': round(min(on), 3),
                              'off_spread': round(max(off) - min(off), 3), 'on_spread': round(max(on) - min(on), 3)}
        result['torch_peak_bytes_beyond_the_input'] = {'off': peak_bytes(False), 'on': peak_bytes(True), 'result_bytes': 3 * H * W * 2}
        print(json.dumps({k: result[k] for k in ('frame_ms', 'torch_peak_bytes_beyond_the_input')}), flush=True)

        # the stream
        steps = [{'op': 'buffer', 'bitDepth': BITS}, {'op': 'DN', 'model': 'lite5', 'strength': STRENGTH}]
        rng = np.random.default_rng(2024)
        warm = b''.join(rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(2))
        timed = b''.join(rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(args.frames))
        sink = []

        def leg(run, data, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = run(io.BytesIO(data).read)
            torch.cuda.synchronize()
            assert got == n
            return time.perf_counter() - t0

        res = {}
        for _ in range(min(3, args.rounds)):
            for name, flag, depth in (('serial_off', False, 0), ('serial_on', True, 0), ('streamed_off', False, 2), ('streamed_on', True, 2)):
                config.filterOnDevice = flag
                del sink[:]
                if depth:
                    stream = procedure.genFrameStream(steps, W, H, depth)
                    run = lambda read: procedure.runFramesStreamed(stream, read, sink.append)
                    edge = stream.edge
                else:
                    process, _ = procedure.genProcess(steps, bitDepth=BITS)
                    run = lambda read: procedure.runFrames(process, read, sink.append, W, H, bitDepth=BITS)
                    edge = None
                leg(run, warm, 2)
                dt = leg(run, timed, args.frames)
                if depth:
                    stream.close()
                r = res.setdefault(name, {'edge': edge, 'fps': []})
                r['fps'].append(round(args.frames / dt, 2))
        for r in res.values():
            r['fps_best'] = max(r['fps'])
            r['fps_spread'] = round(max(r['fps']) - min(r['fps']), 2)
        result['stream'] = res
    finally:
        config.filterOnDevice = True
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
