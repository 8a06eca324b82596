"""The JSON line bench.py prints is a contract with the driver (metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
vs_baseline / dtype / data / config + the roofline and cpu_baseline objects).  bench.py itself needs the GPU; here the lines committed under profiles/ (the
closing pass of the latest round) are held against that contract and against BASELINE.json, so that a change of the line's shape shows up on CPU."""
import glob
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = json.load(open(os.path.join(ROOT, 'BASELINE.json')))
ROUNDS = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]')))


def _line(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def _latest(name):
    for d in reversed(ROUNDS):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return None


def test_headline_line_follows_the_contract():
    p = _latest('bench_c2.json')
    if p is None:
        pytest.skip('no committed bench line')
    r = _line(p)
    for k, t in (('metric', str), ('value', (int, float)), ('unit', str), ('n_gpus', int), ('steps', int), ('warmup', int), ('ms_per_step', (int, float)),
                 ('higher_is_better', bool), ('scaling', str), ('dtype', str), ('data', str), ('config', dict), ('roofline', dict), ('cpu_baseline', dict)):
        assert k in r and isinstance(r[k], t), k
    assert 'vs_baseline' in r and r['vs_baseline'] is None          # BASELINE.md holds no published number for this metric on this hardware
    # BASELINE.json: "megapixels/sec, 1080p -> 4K 4x SR (... a4), tiled" -- the line names the same metric on the same config (a4 is Net4x: SURVEY.md section 8)
    assert BASE['metric'].startswith('megapixels/sec') and r['metric'].startswith('megapixels/sec') and r['unit'] == 'MP/s'
    assert all(w in r['metric'] for w in ('1080p', '4x', 'a4')) and all(w in BASE['metric'] for w in ('1080p', 'a4')), (r['metric'], BASE['metric'])
    assert r['higher_is_better'] is True and r['scaling'] == 'weak' and r['n_gpus'] == 1 and r['data'].startswith('synthetic')
    assert isinstance(r['config'].get('workload'), str) and 'model' not in r['config']
    assert abs(r['value'] - 1920 * 1080 / 1e6 / (r['ms_per_step'] / 1e3)) / r['value'] < 2e-3      # value = input megapixels of the frame over the step time
    rf = r['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in rf, k
    assert rf['bound'] in ('hbm', 'mfma') and rf['unit'] in ('GB/s', 'TFLOP/s')
    assert abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-3 and 0 < rf['frac'] < 1
    assert rf['traffic'] is None or rf['traffic'] > 0
    cb = r['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in cb, k
    assert cb['kind'] in ('reference', 'port') and cb['unit'] == r['unit'] and cb['cores'] >= 1
    par = r['config'].get('parity_max_abs_vs_oracle')
    assert par is not None and par <= r['config']['parity_tolerance'] == 1e-3 and r['config']['parity_ok'] is True
    # round 5: the other BASELINE configs ride on the default command's line (children of it), the split-operand layers are an MFMA object, the drop-in loop is taken apart
    if 'configs' in r:
        for c in (3, 4, 5):
            e = r['configs']['config%d' % c]
            assert 'error' not in e, e
            assert e['ms_per_step'] > 0 and e['value'] > 0 and e['parity_ok'] is True and e['parity_max_abs_vs_oracle'] <= 1e-3
            assert 'configs[%d]' % (c - 1) in e['workload']
        so = r['roofline_split_operand']
        assert so['bound'] == 'mfma' and so['unit'] == 'TFLOP/s' and abs(so['frac'] - so['achieved'] / so['peak']) < 1e-3
        assert rf.get('traffic_source') in (None, 'this run', 'committed')
        d = r['dropin_loop']
        assert d['breakdown']['engine_forwards_only_ms'] > 0 and d['with_moe_blend_tile']['ms_per_step'] <= d['ms_per_step'] * 1.02


@pytest.mark.parametrize('cfg', [3, 4, 5])
def test_other_config_lines_follow_the_contract(cfg):
    p = _latest('bench_c%d.json' % cfg)
    if p is None:
        pytest.skip('no committed line for config %d' % cfg)
    r = _line(p)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
        assert k in r, k
    assert r['n_gpus'] == 1 and r['higher_is_better'] is True and r['vs_baseline'] is None
    assert 'configs[%d]' % (cfg - 1) in r['config']['workload']
    assert r['config'].get('parity_ok') is True and r['config']['parity_max_abs_vs_oracle'] <= 1e-3


def test_pmc_summary_names_its_tree():
    p = os.path.join(ROOT, 'profiles', 'pmc_bench.json')
    if not os.path.exists(p):
        pytest.skip('no PMC summary')
    d = json.load(open(p))
    assert isinstance(d.get('source_sha256'), str) and len(d['source_sha256']) == 64
    for g in ('convt_R1.up1', 'u.up1', 'arsb', 'exact'):            # the groups bench.py looks its `traffic` fields up under
        assert g in d['groups'] and d['groups'][g]['hbm_bytes_per_frame'] > 0, g


def test_dump_outputs_is_a_fixed_bounded_sample_of_the_canvas(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last step's fp16 canvas (3 x 4320 x 7680) as float32 / float64 .npy files -- the same positions in every run, every
    element inside the row / column sums, all files of all ranks of one node within 64 MB."""
    import numpy as np
    import torch
    import bench
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    y = torch.rand((3, 4320, 7680), generator=torch.Generator().manual_seed(0)).half()
    bench._dump_outputs(str(tmp_path / 'a'), y)
    bench._dump_outputs(str(tmp_path / 'b'), y.clone())
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['canvas_col_sums.npy', 'canvas_row_sums.npy', 'canvas_sample.npy', 'canvas_window.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= bench.DUMP_BYTES
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    top, left, side = bench.DUMP_WINDOW
    assert np.array_equal(np.load(tmp_path / 'a' / 'canvas_window.npy'), y[:, top:top + side, left:left + side].float().numpy())
    y[2, 4000, 7000] += 0.5                     # one element that neither the sample nor the window needs to hold
    bench._dump_outputs(str(tmp_path / 'c'), y)
    for n in ('canvas_row_sums.npy', 'canvas_col_sums.npy'):
        assert not np.array_equal(np.load(tmp_path / 'a' / n), np.load(tmp_path / 'c' / n)), n
    # --gpus 8: each rank writes the frame it stitched, within an eighth of the budget
    monkeypatch.setenv('WORLD_SIZE', '8')
    bench._dump_outputs(str(tmp_path / 'r'), {5: y})
    names = sorted(os.listdir(tmp_path / 'r'))
    assert names == ['frame5_col_sums.npy', 'frame5_row_sums.npy', 'frame5_sample.npy', 'frame5_window.npy']
    assert sum(os.path.getsize(tmp_path / 'r' / n) for n in names) <= bench.DUMP_BYTES // 8
    # --gpus 16 --strong: {frame: (first row, row band)}; a rank whose band holds no rows writes nothing
    monkeypatch.setenv('WORLD_SIZE', '16')
    bench._dump_outputs(str(tmp_path / 's'), {0: (1080, y[:, 1080:1350])})
    names = sorted(os.listdir(tmp_path / 's'))
    assert names == ['frame0_rows1080_1350_col_sums.npy', 'frame0_rows1080_1350_row_sums.npy', 'frame0_rows1080_1350_sample.npy', 'frame0_rows1080_1350_window.npy']
    assert np.array_equal(np.load(tmp_path / 's' / 'frame0_rows1080_1350_row_sums.npy'), np.load(tmp_path / 'c' / 'canvas_row_sums.npy')[:, 1080:1350])
    bench._dump_outputs(str(tmp_path / 'e'), {0: (4320, y[:, 4320:])})
    assert os.listdir(tmp_path / 'e') == []
    bench._dump_outputs(str(tmp_path / 'f'), {3: y})     # a full canvas: 16 ranks' files still fit DUMP_BYTES
    assert sum(os.path.getsize(tmp_path / 'f' / n) for n in os.listdir(tmp_path / 'f')) <= bench.DUMP_BYTES // 16
