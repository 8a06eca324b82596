"""SEDN under MOE_PREC_AUTO: the checkpoint is measured when it is loaded (calibrate_sedn in csrc/calibrate.cpp, run by moe_net_finalize) -- plain fp16 where that
holds the 1e-3 contract on THESE weights, 'fp16x3' where it does not.  Needs a HIP device: `pytest -m gpu`.

The real l15 / l25 / l50 files are not in the zoo mount; the synthetic l25 of golden_defs stands in for "a checkpoint fp16 is fine for", and the same checkpoint with
rblock.4 (the 64 -> 256 conv of every block) scaled by S for "one it is not fine for".  Choosing S (nobody had measured it): an emulation on the CPU (the oracle's
forward with every conv's operands rounded to fp16, the fused block tail's folded weights rounded once, 64 x 64 corner of the tile below) gave 3.8e-4 / 6.6e-4 /
1.29e-3 / 5.6e-3 for S = 1 / 1.25 / 1.5 / 2 (and 2e-1 for 3; all three rblock convs scaled: 5e-3 already at 1.25, the net diverges from 1.5 on).  The full tile is a
maximum over sixteen times as many values and the engine's fp16 sits above the emulation on the checkpoint as shipped (4-6e-4 against 3.8e-4), so S = 1.5 -- the
smallest of 1.25, 1.5, 2.0, 3.0 the emulation puts above 1.2e-3 -- is the factor; scaling rblock.4 alone is enough.  The value of (a) on the GPU has not been recorded here yet: the test prints it and writes it to the report.

Bounds: 1e-3 is the contract (against oracle.nets, fp32); 8.5e-4 the calibration's target (kCalibTarget); 2e-5 what 'fp16x3' is pinned to elsewhere.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd.weights import load_state_dict_file
from oracle import nets as onets
from test_gpu_fullsize import _report
from test_gpu_parity import dev, module_for  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-3
TARGET = 8.5e-4           # kCalibTarget
S = 1.5                   # rblock.4 of every block x S: see the module docstring
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _l25(s=1.0):
    sd = gd.state_dict_for('l25', load_state_dict_file)
    if s == 1.0:
        return sd
    return {k: (np.ascontiguousarray(v * np.float32(s)) if k.endswith('rblock.4.weight') else v) for k, v in sd.items()}


def _module(sd, precision='auto', pre=None):
    from moephoto_amd import models
    m = models.SEDN()
    m.precision = precision
    if pre:
        pre(m)
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for n, v in sd.items()})
    return m.eval().to(dtype=torch.float32, device='cuda:0')


def _stub_sedn():
    """class SEDN of INTEGRATION.md's binding, executed as written (the library path filled in)"""
    from moephoto_amd import _lib
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    code = re.search(r'```python\n(.*?)```', text, re.S).group(1).replace("'libmoephoto_amd.so'", repr(_lib.LIB_PATH))
    ns = {}
    exec(compile(code, 'INTEGRATION.md', 'exec'), ns)
    return ns['SEDN']


def _tile():
    return gd.noise_u8(5, (3, 256, 256)).astype(np.float32)[:, None] / np.float32(255)


def _err(m, x, want, dev):
    return float(np.abs(m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy() - want).max())


def _sweep(m16, mx3, dev, seeds=(0, 1, 2, 3, 4, 5, 6, 7)):
    """worst plane-tile of len(seeds) x 3 uint8-noise plane-tiles of 256 x 256, fp16 against fp16x3"""
    per = []
    for seed in seeds:
        xd = torch.from_numpy(gd.noise_u8(seed, (3, 256, 256)).astype(np.float32)[:, None] / np.float32(255)).to(dev)
        per += (m16(xd)[-1] - mx3(xd)[-1]).abs().amax(dim=(1, 2, 3)).tolist()
    return per


def test_auto_moves_a_checkpoint_that_breaks_fp16_to_fp16x3(dev):
    """l25 with rblock.4 x 1.5, on the full 256 x 256 uint8-noise tile against the fp32 oracle.  (a) finalized with the explicit 'fp16' it is > 1e-3 away: the
    checkpoint is a real hazard for SEDN's default arithmetic (its value is printed and reported); (b) loaded through the INTEGRATION.md stub as written -- MOE_PREC_AUTO -- it is
    within 1e-3 and the net says it runs in 'fp16x3'; the fallback itself ('fp16x3' explicit) is within 1e-3 too.  Without the measurement at finalize (b) fails with
    (a)'s error."""
    from moephoto_amd import _lib
    sd = _l25(S)
    x = _tile()
    want = onets.forward('sedn', sd, x).numpy()
    ea = _err(_module(sd, 'fp16'), x, want, dev)
    ex = _err(_module(sd, 'fp16x3'), x, want, dev)
    m = _stub_sedn()()
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for n, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(False)
    m.eval()
    m = m.to(dtype=torch.float32, device=dev)
    eb = _err(m, x, want, dev)
    resolved = _lib.lib().moe_net_resolved_precision(m.h, _lib.PREC_AUTO)
    mm = _module(sd)
    em = _err(mm, x, want, dev)
    print('rblock.4 x {}: fp16 {:.3e}, fp16x3 {:.3e}, AUTO through the stub {:.3e} (resolved {}), EngineModule auto {:.3e} ({})'.format(S, ea, ex, eb, resolved, em, mm.resolved_precision()))
    _report('sedn_calibrate_perturbed', {'S': S, 'fp16': ea, 'fp16x3': ex, 'auto_stub': eb, 'auto_module': em, 'resolved': mm.resolved_precision()})
    assert ea > TOL, 'precondition: explicit fp16 should break the contract on this checkpoint: {:.3e}'.format(ea)
    assert ex <= TOL, 'the fallback arithmetic itself: {:.3e}'.format(ex)
    assert eb <= TOL, 'AUTO through the INTEGRATION.md stub vs the oracle: {:.3e}'.format(eb)
    assert resolved == _lib.PRECISIONS['fp16x3']
    assert em <= TOL and mm.resolved_precision() == 'fp16x3' and mm.exact_blocks() == 0


def test_nothing_changes_for_the_checkpoint_that_ships(dev):
    """The synthetic l25 as shipped under AUTO: 'fp16', bit for bit the explicit 'fp16' on a small and a full-size noise image, within 1e-3 of the oracle."""
    sd = _l25()
    ma, mf = _module(sd), _module(sd, 'fp16')
    assert ma.resolved_precision() == 'fp16' and ma.exact_blocks() == 0
    n, err = ma.calibrate()
    assert n == 0 and 0 < err <= TARGET * 1.05, (n, err)
    assert ma.resolved_precision() == 'fp16'
    for shape in ((3, 24, 40), (3, 256, 256)):
        x = gd.noise_image(25, shape)[:, None]
        xd = torch.from_numpy(x).to(dev)
        ya = ma(xd)[-1]
        assert torch.equal(ya, mf(xd)[-1]), shape
        e = float(np.abs(ya.cpu().numpy() - onets.forward('sedn', sd, x).numpy()).max())
        print('l25 as shipped, AUTO, noise {}: {:.3e} vs the oracle (predicted full-frame worst tile {:.3e})'.format(shape, e, err))
        assert e <= TOL, (shape, e)
    assert torch.equal(module_for('l25')(xd)[-1], ya)


def test_auto_calibrate_off_is_the_opt_out_and_a_new_checkpoint_is_measured_again(dev):
    """Option auto_calibrate = 0 keeps plain fp16 on the perturbed checkpoint, unmeasured (the documented opt-out); moe_net_calibrate on that net reports a predicted
    error above the target and leaves its arithmetic alone.  Loading other weights (moe_net_set_param) invalidates a measurement: the same module given the shipped
    checkpoint runs in 'fp16' again, and given the perturbed one falls back again."""
    sd_bad, sd_ok = _l25(S), _l25()
    m0 = _module(sd_bad, pre=lambda q: q.set_option('auto_calibrate', 0))
    assert m0.resolved_precision() == 'fp16'
    n, err = m0.calibrate()
    assert n == 0 and err > TARGET * 1.05, (n, err)
    assert m0.resolved_precision() == 'fp16'          # (auto_calibrate = 0: the figure is reported, the opt-out stands)
    x = torch.from_numpy(_tile()).to(dev)
    assert torch.equal(m0(x)[-1], _module(sd_bad, 'fp16')(x)[-1])
    m = _module(sd_bad)
    assert m.resolved_precision() == 'fp16x3'
    y_bad = m(x)[-1].clone()
    m.load_state_dict({n_: torch.from_numpy(np.ascontiguousarray(v)) for n_, v in sd_ok.items()})
    m.to(dtype=torch.float32, device=dev)
    assert m.resolved_precision() == 'fp16' and torch.equal(m(x)[-1], _module(sd_ok, 'fp16')(x)[-1])
    m.load_state_dict({n_: torch.from_numpy(np.ascontiguousarray(v)) for n_, v in sd_bad.items()})
    m.to(dtype=torch.float32, device=dev)
    assert m.resolved_precision() == 'fp16x3' and torch.equal(m(x)[-1], y_bad)
    # an explicit arithmetic is nobody's business but the caller's: the measurement reports and changes nothing
    mx = _module(sd_bad, 'fp16x3')
    n, err2 = mx.calibrate()
    assert n == 0 and err2 == pytest.approx(err, rel=1e-3) and mx.resolved_precision() == 'fp16x3' and torch.equal(mx(x)[-1], y_bad)


def test_lite_has_no_knob_and_mixed_stays_refused_for_sedn(dev):
    from moephoto_amd import _lib, models
    L = _lib.lib()
    m = module_for('lite2')
    assert m.calibrate() is None
    n, e = ctypes.c_int(7), ctypes.c_double(7.0)
    _lib.check(L.moe_net_calibrate(m._h, 0.0, ctypes.byref(n), ctypes.byref(e), None))
    assert n.value == 0 and e.value == 0.0
    s = models.SEDN()
    s.load_state_dict({k: torch.from_numpy(v) for k, v in _l25().items()})
    assert L.moe_net_finalize(s._h, 0, _lib.PRECISIONS['mixed']) == _lib.EINVAL and b'MOE_PREC_MIXED' in L.moe_last_error()
    assert L.moe_abi_version() == 4


@pytest.mark.parametrize('s', [1.0, S])
def test_predicted_error_bounds_the_swept_error(s, dev):
    """The figure the decision is taken on (measured on twelve tiles x kCalibInflateSEDN) is at least the worst of 24 other uint8-noise plane-tiles of 256 x 256,
    fp16 against fp16x3 -- for the checkpoint that ships and for the perturbed one."""
    sd = _l25(s)
    m16, mx3 = _module(sd, 'fp16'), _module(sd, 'fp16x3')
    _, predicted = m16.calibrate()
    per = _sweep(m16, mx3, dev)
    assert len(per) >= 24
    print('rblock.4 x {}: predicted {:.3e}, worst of {} plane-tiles {:.3e}'.format(s, predicted, len(per), max(per)))
    _report('sedn_calibrate_predicted_vs_swept_x{}'.format(s), {'predicted': predicted, 'swept_worst': max(per), 'plane_tiles': len(per)})
    assert predicted >= max(per), (s, predicted, max(per))


@pytest.mark.parametrize('key', ['dn_lite5', 'dn_lite10', 'dn_lite15'])
def test_dn_lite_full_size_tiles_vs_oracle(key, dev):
    """NetDN at the size that ships, against the ORACLE (the all-tile sweep of test_gpu_fullsize compares the engine with its own exact mode): four uint8-noise tiles of
    3 x 256 x 256 per key under AUTO, each within 1e-3."""
    m = module_for(key)
    sd = gd.state_dict_for(key, load_state_dict_file)
    errs = []
    for seed in (0, 1, 2, 3):
        x = gd.noise_u8(seed, (3, 256, 256)).astype(np.float32)[:, None] / np.float32(255)
        errs.append(_err(m, x, onets.forward('netdn', sd, x).numpy(), dev))
    print('{} ({} / {} blocks): {}'.format(key, m.resolved_precision(), m.exact_blocks(), ['{:.3e}'.format(e) for e in errs]))
    _report('dn_lite_fullsize_vs_oracle_' + key, {'precision': m.resolved_precision(), 'exact_blocks': m.exact_blocks(), 'worst': max(errs), 'per_tile': errs})
    assert max(errs) <= TOL, (key, errs)
