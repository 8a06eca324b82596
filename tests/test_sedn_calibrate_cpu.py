"""SEDN's load-time measurement, the parts that need no GPU: the entry point's argument checks, and the multi-rank agreement (moephoto_amd/dist.py::agree_arithmetic,
world size 2 under gloo with stand-in modules, as tests/test_dist_cpu.py does for the ARSB nets)."""
import ctypes
import os
import socket
import subprocess
import sys

import pytest

from moephoto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calibrate_on_an_unfinalized_sedn_net_is_refused_before_any_device_work():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_SEDN, 1, ctypes.byref(h)))
    try:
        n, e = ctypes.c_int(7), ctypes.c_double(7.0)
        assert L.moe_net_calibrate(h, 0.0, ctypes.byref(n), ctypes.byref(e), None) == _lib.ESTATE and b'finalized' in L.moe_last_error()
        assert (n.value, e.value) == (7, 7.0)
        assert L.moe_net_calibrate(None, 0.0, ctypes.byref(n), ctypes.byref(e), None) == _lib.EINVAL
        assert L.moe_net_exact_blocks(h) == 0
        assert L.moe_net_resolved_precision(h, _lib.PREC_AUTO) == _lib.PRECISIONS['fp16']        # (the family's default until a finalize has measured the weights)
        assert L.moe_net_finalize(h, 0, _lib.PRECISIONS['mixed']) == _lib.EINVAL and b'MOE_PREC_MIXED' in L.moe_last_error()
        assert L.moe_net_set_option(h, b'auto_calibrate', b'0') == 0
        assert L.moe_abi_version() == 4
    finally:
        L.moe_net_destroy(h)


WORKER = r'''
import os, sys
sys.path.insert(0, os.environ['MOE_ROOT'])
import torch.distributed as dist
from moephoto_amd import dist as mdist
dist.init_process_group('gloo')
rank = dist.get_rank()
class _SEDN(object):
    """EngineModule's arithmetic surface for a SEDN net: 'auto' resolves to what the rank's own measurement settled on; an explicit precision is itself"""
    def __init__(self, measured): self.precision, self.measured, self._finalized_key, self.calls = 'auto', measured, (0, 'auto'), []
    def resolved_precision(self): return self.measured if self.precision == 'auto' else self.precision
    def exact_blocks(self): return 0
    def set_precision(self, p): self.calls.append(p); self.precision = p; self._finalized_key = (0, p); return self
    def set_exact_blocks(self, b): raise AssertionError('SEDN has no block count to impose')
# rank 0 fell back, the other rank's measurement kept fp16 (another driver, another device generation): every rank runs fp16x3 -- the other one by an explicit finalize
m = _SEDN('fp16x3' if rank == 0 else 'fp16')
assert mdist.agree_arithmetic(m) == ('fp16x3', 0) and m.resolved_precision() == 'fp16x3'
assert m.calls == ([] if rank == 0 else ['fp16x3']), (rank, m.calls)
assert mdist.agree_arithmetic(m) == ('fp16x3', 0) and len(m.calls) <= 1          # (cached: no second collective)
# the other way round: rank 0 kept fp16, the other rank fell back -> fp16 everywhere
m = _SEDN('fp16' if rank == 0 else 'fp16x3')
assert mdist.agree_arithmetic(m) == ('fp16', 0) and m.resolved_precision() == 'fp16'
assert m.calls == ([] if rank == 0 else ['fp16'])
# agreement from the start: nothing is imposed
m = _SEDN('fp16x3')
assert mdist.agree_arithmetic(m) == ('fp16x3', 0) and m.calls == []
dist.barrier()
print('rank', rank, 'ok')
'''


def test_a_sedn_fallback_on_rank_0_puts_every_rank_into_fp16x3(tmp_path):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / 'worker.py'
    script.write_text(WORKER)
    procs = []
    for rank in range(2):
        env = dict(os.environ, MOE_ROOT=ROOT, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', OMP_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=180)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and 'ok' in out, 'rank {}:\n{}'.format(rank, out)
