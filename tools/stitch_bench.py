#!/usr/bin/env python
"""Device time of the three stitch edges on synthetic pools (measurement tool; results: profiles/stitch/summary.md).

    python tools/stitch_bench.py [--lib LIB.so] [--tag NAME] [--reps 50] [--append FILE.jsonl]      one round: a fresh process per library
    python tools/stitch_bench.py --report FILE.jsonl [--base TAG] [--out FILE.json]                 fastest and spread per tag and case

Device events around `reps` back-to-back repetitions, per repetition, in microseconds.  A comparison of two libraries alternates rounds of both inside ONE job (machines
differ by several per cent); a case holds when the new fastest time is no more than the base's fastest plus the base's own spread (max - min over its rounds).

cases   canvas_8k        moe_stitch       fp16 canvas 3 x 4320 x 7680 (x4 of 1080p, tiles of 256)
        samples_8k       moe_stitch_out   u16 samples of the same canvas
        mix_canvas_1080  moe_stitch_mix   fp16, strength 0.6, 3 x 1080 x 1920 (tiles of 256), canvas form
        mix_sample_1080  moe_stitch_mix   the same, u16 samples
        canvas_w3836     moe_stitch       fp16 canvas 3 x 2160 x 3836 (out_w % 8 == 4)
        canvas_w1923     moe_stitch       fp16 canvas 3 x 1080 x 1923 (odd)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def report(path, base, out):
    rounds = {}
    for line in open(path):
        if line.strip():
            r = json.loads(line)
            for case, us in r['us'].items():
                rounds.setdefault(case, {}).setdefault(r['tag'], []).append(us)
    res = {}
    for case, tags in rounds.items():
        res[case] = {t: {'rounds_us': v, 'fastest_us': min(v), 'spread_us': round(max(v) - min(v), 2)} for t, v in tags.items()}
        if base in tags:
            bar = res[case][base]['fastest_us'] + res[case][base]['spread_us']
            for t in tags:
                if t != base:
                    res[case][t]['holds'] = res[case][t]['fastest_us'] <= bar
        print(case, {t: (v['fastest_us'], v['spread_us'], v.get('holds')) for t, v in res[case].items()})
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, 'w'), indent=1)
    return 0 if all(v.get('holds', True) for c in res.values() for v in c.values()) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib')
    ap.add_argument('--tag', default='tree')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--append')
    ap.add_argument('--report')
    ap.add_argument('--base', default='parent')
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.report:
        sys.exit(report(args.report, args.base, args.out))

    import torch
    from moephoto_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from moephoto_amd.imageProcess import TilePlan
    _lib.require_device()
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

    def plan_pool(shape, sc, pad, crop):
        pl = TilePlan(shape, 1 << 40, 1e-3, pad, sc, 8, crop)
        return pl, torch.rand(pl.pool_elems(shape[0]), dtype=torch.float32, device=dev)

    us = {}
    pl, pool = plan_pool((3, 1080, 1920), 4, 5, 256)
    canvas = torch.empty((3, pl.outH, pl.outW), dtype=torch.float16, device=dev)
    samples = torch.empty((pl.outH, pl.outW, 3), dtype=torch.int16, device=dev)
    us['canvas_8k'] = device_us(lambda: _lib.check(L.moe_stitch(pl._h, 0, pool.data_ptr(), None, 3, canvas.data_ptr(), _lib.F16, st)))
    us['samples_8k'] = device_us(lambda: _lib.check(L.moe_stitch_out(pl._h, 0, pool.data_ptr(), None, 3, _lib.F16, 16, samples.data_ptr(), _lib.U16, st)))
    del pool, canvas, samples

    pl, pool = plan_pool((3, 1080, 1920), 1, 7, 256)
    inp = torch.rand((3, pl.outH, pl.outW), dtype=torch.float32, device=dev).half()
    sC, sH, sW = inp.stride()
    for name, bits, dst, dt in (('mix_canvas_1080', 0, torch.empty_like(inp), _lib.F16), ('mix_sample_1080', 16, torch.empty((pl.outH, pl.outW, 3), dtype=torch.int16, device=dev), _lib.U16)):
        us[name] = device_us(lambda: _lib.check(L.moe_stitch_mix(pl._h, 0, pool.data_ptr(), None, 3, inp.data_ptr(), _lib.F16, sC, sH, sW, None, 0, 0, 0.6, bits, dst.data_ptr(), dt, st)))
    del pool, inp

    for name, shape in (('canvas_w3836', (3, 2160, 3836)), ('canvas_w1923', (3, 1080, 1923))):
        pl, pool = plan_pool(shape, 1, 7, 256)
        assert pl.outW == shape[2]
        canvas = torch.empty((3, pl.outH, pl.outW), dtype=torch.float16, device=dev)
        us[name] = device_us(lambda: _lib.check(L.moe_stitch(pl._h, 0, pool.data_ptr(), None, 3, canvas.data_ptr(), _lib.F16, st)))
        del pool, canvas

    line = json.dumps({'tag': args.tag, 'reps': args.reps, 'us': us})
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
        open(args.append, 'a').write(line + '\n')


if __name__ == '__main__':
    main()
