#!/usr/bin/env python
"""What the frame stream's reuse costs and what it buys (measurement tool; results: profiles/reuse/summary.md).  1080p 16-bit frames, a2 -> 4K and a4 -> 8K, ring depth 2.

    python tools/reuse_bench.py cost   [--root DIR] [--models a2,a4] [--frames 32] [--warmup 4] [--rounds 3] [--out FILE.json]
    python tools/reuse_bench.py versus PARENT_TREE [--models ..] [--frames ..] [--rounds 3] [--limit 300] [--out FILE.json]
    python tools/reuse_bench.py gain   [--models ..] [--frames ..] [--warmup ..] [--rounds 3] [--out FILE.json]
    python tools/reuse_bench.py kernel [--out FILE.json]
    python tools/reuse_bench.py where  [--models a2] [--frames ..] [--rounds 3] [--out FILE.json]
    (every mode but kernel: --depth N, the ring depth, default 2)

cost    distinct noise frames (nothing to reuse) through genFrameStream in ONE process: the forms the tree has -- `plain`, and `reuse` where genFrameStream takes the
        argument -- alternate `rounds` times; a leg is `warmup` untimed frames and `frames` frames between two host clock reads, the second behind a device synchronise,
        with the ring's per-stage times beside it (tools/frame_stream_bench.py's conventions).  --root: the tree whose package is measured (default: this one), so the
        same file measures a checkout of the parent commit, which has `plain` alone
versus  the driver of the comparison against the parent: `cost` of PARENT_TREE and of this tree as alternating child processes, `rounds` of each, every child under
        its own time limit (`timeout -k 10 LIMIT`), nothing started after one that failed.  Prints, per model, every leg's fps and compute-stage ms, the parent's own
        leg-to-leg spread over the whole call and the differences of this tree's two forms against the parent's median
gain    reuse=True on four sequences -- all_new; twice (every frame shown twice); patch (a static frame with a 256 x 256 patch of fresh noise moving 64 px per frame);
        top_third (a static frame whose top third is fresh in every frame) -- alternating `rounds` times: the fraction of plane-tile pixels run (stream.reuse), the
        compute-stage ms and the fps of each
kernel  moe_changed_blocks alone on a 1080p bgr48le and a 1080p yuv420p10le frame (equal frames: two reads per byte; wholly different frames: a write more), against
        moe_to_float and moe_planes_to_float on the same frames, from device events around 50 calls
where   the reuse stream on distinct frames taken apart, alternating legs in one process: plain; reuse; reuse without the detector and the map's copy (the map
        forced to "all changed"); the same without the compute stage's host wait for `uploaded` as well -- which of the three additions the time goes to

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
H, W, BITS, CROP, DEPTH = 1080, 1920, 16, 256, 2          # (DEPTH: the ring depth, --depth)


def _setup(root):
    for p in (root, os.path.join(root, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import golden_defs as gd
    from moephoto_amd import _lib, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _lib.require_device()
    config.modelRoot, config.deviceId, config.fp16, config.crop_sr, config.ensembleSR = gd.ZOO, 0, True, CROP, 0
    tmp = tempfile.mkdtemp(prefix='moe_reuse_bench_')
    wpath = os.path.join(tmp, 'a4.pth')
    save_state_dict_file(gd.synth_state_dict('a4', load_state_dict_file), wpath)
    runSR.mode_switch['a4'] = (wpath, runSR.mode_switch['a4'][1])
    return tmp


def _steps(key):
    return [{'op': 'buffer', 'bitDepth': BITS}, {'op': 'SR', 'model': key[:-1], 'scale': int(key[-1]), 'ensemble': 0}]


def _leg(stream, frames, warmup):
    """warmup untimed frames, then the rest between two host clock reads -> (fps, the ring's stage ms per frame, stream.reuse of the timed frames or None)"""
    import torch
    from moephoto_amd import procedure
    sink = {'n': 0}

    def write(buf):
        sink['n'] += 1

    def run(data, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = procedure.runFramesStreamed(stream, io.BytesIO(data).read, write)
        torch.cuda.synchronize()
        assert got == n, (got, n)
        return time.perf_counter() - t0
    if warmup:
        run(b''.join(frames[:warmup]), warmup)
    for k in stream.backend.stats:
        stream.backend.stats[k] = 0
    counters = getattr(stream, 'reuse', None)
    if counters is not None:
        counters['pixels_planned'] = counters['pixels_run'] = 0
    n = len(frames) - warmup
    dt = run(b''.join(frames[warmup:]), n)
    st = stream.backend.stats
    stages = {k: round(v / max(1, st['frames']), 3) for k, v in st.items() if k != 'frames'}
    frac = round(counters['pixels_run'] / max(1, counters['pixels_planned']), 4) if counters is not None else None
    return round(n / dt, 3), stages, frac


def _noise(rng, n):
    import numpy as np
    return [rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(n)]


def cost(args):
    import inspect
    import numpy as np
    root = os.path.abspath(args.root or HERE)
    tmp = _setup(root)
    from moephoto_amd import procedure
    forms = ['plain'] + (['reuse'] if 'reuse' in inspect.signature(procedure.genFrameStream).parameters else [])
    frames = _noise(np.random.default_rng(2024), args.warmup + args.frames)
    result = {'root': root, 'forms': forms, 'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'models': {}}
    for key in args.models.split(','):
        res = {f: {'fps': [], 'compute_ms': [], 'stage_ms_per_frame': []} for f in forms}
        for _ in range(args.rounds):
            for f in forms:
                stream = procedure.genFrameStream(_steps(key), W, H, DEPTH, timing=True, **({'reuse': True} if f == 'reuse' else {}))
                fps, stages, frac = _leg(stream, frames, args.warmup)
                stream.close()
                res[f]['fps'].append(fps)
                res[f]['compute_ms'].append(stages['compute_ms'])
                res[f]['stage_ms_per_frame'].append(stages)
                if frac is not None:
                    res[f].setdefault('fraction_run', []).append(frac)
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def _emit(result, out):
    print(json.dumps(result), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(result, open(out, 'w'), indent=1)


def versus(args):
    parent = os.path.abspath(args.parent)
    legs = []
    for r in range(args.rounds):
        for name, root in (('parent', parent), ('tree', HERE)):
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), 'cost', '--root', root, '--models', args.models,
                   '--frames', str(args.frames), '--warmup', str(args.warmup), '--depth', str(DEPTH), '--rounds', '1' if name == 'tree' else '2']
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit('reuse_bench versus: the {} child of round {} ended with status {}; nothing more is started'.format(name, r, p.returncode))
            legs.append((name, json.loads(p.stdout.strip().splitlines()[-1])))
    out = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'order': [n for n, _ in legs], 'models': {}}
    med = lambda v: sorted(v)[len(v) // 2]
    for key in args.models.split(','):
        m = {}
        for form, who, f in (('parent', 'parent', 'plain'), ('plain', 'tree', 'plain'), ('reuse', 'tree', 'reuse')):
            got = [res['models'][key][f] for n, res in legs if n == who]
            m[form] = {'fps': sum((g['fps'] for g in got), []), 'compute_ms': sum((g['compute_ms'] for g in got), []),
                       'stage_ms_per_frame': sum((g['stage_ms_per_frame'] for g in got), [])}
        for form in m:
            m[form]['fps_median'], m[form]['compute_ms_median'] = med(m[form]['fps']), med(m[form]['compute_ms'])
        p = m['parent']
        m['parent_spread'] = {'fps': round(max(p['fps']) - min(p['fps']), 3), 'compute_ms': round(max(p['compute_ms']) - min(p['compute_ms']), 3)}
        for form in ('plain', 'reuse'):
            m[form]['against_parent'] = {'fps': round(m[form]['fps_median'] - p['fps_median'], 3), 'compute_ms': round(m[form]['compute_ms_median'] - p['compute_ms_median'], 3)}
            m[form]['inside_parent_spread'] = bool(-m[form]['against_parent']['fps'] <= m['parent_spread']['fps'] and
                                                   m[form]['against_parent']['compute_ms'] <= m['parent_spread']['compute_ms'])
        out['models'][key] = m
    _emit(out, args.out)


def _sequences(n):
    """name -> n frames of 1080p 16-bit"""
    import numpy as np
    rng = np.random.default_rng(7)
    new = lambda: rng.integers(0, 1 << BITS, (H, W, 3), dtype=np.uint16)
    seqs = {'all_new': [new().tobytes() for _ in range(n)]}
    twice = [new().tobytes() for _ in range((n + 1) // 2)]
    seqs['twice'] = [twice[k // 2] for k in range(n)]
    base, patch, top = new(), [], []
    for k in range(n):
        f = base.copy()
        x0, y0 = (64 * k) % (W - 256), (64 * (64 * k // (W - 256))) % (H - 256)
        f[y0:y0 + 256, x0:x0 + 256] = rng.integers(0, 1 << BITS, (256, 256, 3), dtype=np.uint16)
        patch.append(f.tobytes())
        g = base.copy()
        g[:H // 3] = rng.integers(0, 1 << BITS, (H // 3, W, 3), dtype=np.uint16)
        top.append(g.tobytes())
    seqs['patch'], seqs['top_third'] = patch, top
    return seqs


def gain(args):
    tmp = _setup(HERE)
    from moephoto_amd import procedure
    seqs = _sequences(args.warmup + args.frames)
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'models': {}}
    for key in args.models.split(','):
        res = {s: {'fps': [], 'compute_ms': [], 'fraction_run': [], 'stage_ms_per_frame': []} for s in seqs}
        for _ in range(args.rounds):
            for s, frames in seqs.items():
                stream = procedure.genFrameStream(_steps(key), W, H, DEPTH, timing=True, reuse=True)
                fps, stages, frac = _leg(stream, frames, args.warmup)
                stream.close()
                res[s]['fps'].append(fps)
                res[s]['compute_ms'].append(stages['compute_ms'])
                res[s]['fraction_run'].append(frac)
                res[s]['stage_ms_per_frame'].append(stages)
        for s in res:
            res[s]['compute_ms_median'] = sorted(res[s]['compute_ms'])[len(res[s]['compute_ms']) // 2]
        full = res['all_new']['compute_ms_median']
        for s in res:          # compute = constant + fraction * (all-new - constant), solved for the constant where the fraction is below one
            fr = res[s]['fraction_run'][0]
            res[s]['constant_ms'] = round((res[s]['compute_ms_median'] - fr * full) / (1 - fr), 3) if fr < 0.999 else None
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def where(args):
    import numpy as np
    tmp = _setup(HERE)
    from moephoto_amd import procedure
    frames = _noise(np.random.default_rng(2024), args.warmup + args.frames)

    class NoCopy(object):
        def copy_(self, *a, **k):
            pass

    def make(key, variant):
        if variant == 'plain':
            return procedure.genFrameStream(_steps(key), W, H, DEPTH, timing=True)
        s = procedure.genFrameStream(_steps(key), W, H, DEPTH, timing=True, reuse=True)
        b = s.backend
        if variant != 'reuse':
            b._detect = lambda slot, stream: None
            for slot in b.slots:
                slot['pin_map'] = NoCopy()
                slot['map_np'][:] = 1
        if variant == 'no_detector_no_host_wait':
            b._regions = lambda slot: b._changed(slot, b.reuse.begin())
        return s
    result = {'frames': args.frames, 'warmup': args.warmup, 'rounds': args.rounds, 'depth': DEPTH, 'models': {}}
    for key in args.models.split(','):
        res = {}
        for _ in range(args.rounds):
            for v in ('plain', 'reuse', 'no_detector', 'no_detector_no_host_wait'):
                stream = make(key, v)
                fps, stages, _ = _leg(stream, frames, args.warmup)
                stream.close()
                r = res.setdefault(v, {'fps': [], 'compute_ms': [], 'h2d_ms': []})
                r['fps'].append(fps)
                r['compute_ms'].append(stages['compute_ms'])
                r['h2d_ms'].append(stages['h2d_ms'])
        result['models'][key] = res
    shutil.rmtree(tmp, ignore_errors=True)
    _emit(result, args.out)


def kernel(args):
    for p in (HERE, os.path.join(HERE, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    from moephoto_amd import _lib
    L = _lib.lib()
    _lib.require_device()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    N = 50

    def timed(f, before=None):
        for _ in range(3):
            if before:
                before()
            f()
        a, b, total = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), 0.0
        for _ in range(N):
            if before:
                before()
            a.record()
            f()
            b.record()
            b.synchronize()
            total += a.elapsed_time(b)
        return total / N * 1e3          # microseconds per call

    out = {}
    nb = H * W * 3 * 2
    cur = torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).to(dev)
    other = torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).to(dev)
    prev = cur.clone()
    cmap = torch.empty((68 * 120 + 34 * 60,), dtype=torch.uint8, device=dev)
    bgr = lambda: _lib.check(L.moe_changed_blocks(cur.data_ptr(), prev.data_ptr(), 1, H, W * 6, 16, 96, cmap.data_ptr(), 0, st))
    us = timed(bgr)
    out['changed_blocks bgr48le equal'] = {'us': round(us, 2), 'bytes': 2 * nb, 'GB_per_s': round(2 * nb / us / 1e3, 1)}
    us = timed(bgr, before=lambda: prev.copy_(other))
    out['changed_blocks bgr48le all different'] = {'us': round(us, 2), 'bytes': 3 * nb, 'GB_per_s': round(3 * nb / us / 1e3, 1)}
    x = torch.empty((3, H, W), dtype=torch.float16, device=dev)
    us = timed(lambda: _lib.check(L.moe_to_float(cur.data_ptr(), _lib.U16, 16, H, W, 3, x.data_ptr(), _lib.F16, 0, st)))
    out['to_float bgr48le -> fp16'] = {'us': round(us, 2), 'bytes': 2 * nb, 'GB_per_s': round(2 * nb / us / 1e3, 1)}
    ny = H * W * 2
    nf = ny * 3 // 2
    curp, otherp = cur[:nf], other[:nf]
    prevp = curp.clone()

    def planar():
        _lib.check(L.moe_changed_blocks(curp.data_ptr(), prevp.data_ptr(), 1, H, W * 2, 16, 32, cmap.data_ptr(), 0, st))
        _lib.check(L.moe_changed_blocks(curp.data_ptr() + ny, prevp.data_ptr() + ny, 2, H // 2, W, 16, 32, cmap.data_ptr() + 68 * 120, 0, st))
    us = timed(planar)
    out['changed_blocks yuv420p10le equal (two calls)'] = {'us': round(us, 2), 'bytes': 2 * nf, 'GB_per_s': round(2 * nf / us / 1e3, 1)}
    us = timed(planar, before=lambda: prevp.copy_(otherp))
    out['changed_blocks yuv420p10le all different (two calls)'] = {'us': round(us, 2), 'bytes': 3 * nf, 'GB_per_s': round(3 * nf / us / 1e3, 1)}
    y, c = torch.empty((1, H, W), dtype=torch.float16, device=dev), torch.empty((2, H // 2, W // 2), dtype=torch.float16, device=dev)
    us = timed(lambda: _lib.check(L.moe_planes_to_float(curp.data_ptr(), 10, H, W, y.data_ptr(), c.data_ptr(), _lib.F16, 0, st)))
    out['to_float_planes yuv420p10le -> fp16'] = {'us': round(us, 2), 'bytes': 2 * nf, 'GB_per_s': round(2 * nf / us / 1e3, 1)}
    _emit({'calls': N, 'timing': 'device events around each call, mean', 'kernels': out}, args.out)


def main():
    global DEPTH
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['cost', 'versus', 'gain', 'kernel', 'where'])
    ap.add_argument('parent', nargs='?')
    ap.add_argument('--root')
    ap.add_argument('--models', default='a2,a4')
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300)
    ap.add_argument('--depth', type=int, default=DEPTH)
    ap.add_argument('--out')
    args = ap.parse_args()
    DEPTH = args.depth
    if args.mode == 'versus' and not args.parent:
        ap.error('versus needs the parent tree')
    {'cost': cost, 'versus': versus, 'gain': gain, 'kernel': kernel, 'where': where}[args.mode](args)


if __name__ == '__main__':
    main()
