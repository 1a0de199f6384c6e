#!/usr/bin/env python
"""What the size queries of the C ABI answer, as a table: ``njode_supported``, ``njode_param_count``,
``njode_workspace_bytes`` and ``njode_plan_bytes`` for every compiled shape and three shapes of the
shape-generic family over a grid of batch sizes, row counts, schedules and the wrapper's flag sets.

A change that must not move any buffer prints the same table before and after:

    NJODE_LIB=/path/to/old/libnjode_hip.so python tools/abi_sizes.py > old.txt
    python tools/abi_sizes.py > new.txt && cmp old.txt new.txt

The record budget is read once per process, so the table is printed for the default budget and, by a
child process, for ``NJODE_REC_BUDGET_GB=0.001``.  The queries launch nothing; without a device the
budget's cap falls back to that of a 288 GB device.
"""
import ctypes
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from njode_amd import _lib                     # noqa: E402
from njode_amd.build import CONFIGS            # noqa: E402

BATCHES = (1, 16, 17, 100, 257, 5000)
ROWS_PER_PATH = (0, 1, 10)
N_TIMES = (1, 10, 100)
N_STEPS = (0, 1, 100, 512, 4096)
L, T, S, P = _lib.C_GET_LOSS, _lib.C_TRAIN, _lib.C_SAVE_BWD, _lib.C_RETURN_PATH
FLAG_SETS = (L, L | S | T, P, P | T, S | T | _lib.C_SCHED_KNOWN | _lib.C_SCHED_TAIL)
TINY_BUDGET = '0.001'


def shapes():
    import gen_envelope
    out = []
    for i, (d, H, DO, nh, W, act, masked, curt, res, rnn) in enumerate(CONFIGS):
        flags = (masked * _lib.F_MASKED | curt * _lib.F_INPUT_CURRENT_T | res * _lib.F_RESIDUAL
                 | rnn * _lib.F_USE_RNN)
        out.append(('cfg{}'.format(i), _lib.NjodeDims(d, H, DO, nh, W if nh else 0, act if nh else 0, flags)))
    two = lambda w, act=_lib.ACT_TANH: (2, (w, w), (act, act))
    out.append(('gen_d3_h9', gen_envelope.dims_of(3, 9, 3, two(33), _lib.F_RESIDUAL)))
    out.append(('gen_masked_d7', gen_envelope.dims_of(7, 7, 7, two(21), _lib.F_RESIDUAL | _lib.F_MASKED)))
    out.append(('gen_pernet_rnn_d5_h10', gen_envelope.dims_of(
        5, 10, 5, (two(48), two(40, _lib.ACT_RELU), two(72)), _lib.F_RESIDUAL | _lib.F_USE_RNN)))
    return out


def table(budget):
    lib = _lib.lib()
    size = ctypes.c_size_t(0)

    def query(fn, *args):
        size.value = 0
        rc = fn(*args, ctypes.byref(size))
        return str(size.value) if rc == 0 else 'rc{}'.format(rc)

    for name, dims in shapes():
        ref = ctypes.byref(dims)
        print('{} budget={} supported={} params={}'.format(name, budget, lib.njode_supported(ref),
                                                           lib.njode_param_count(ref)))
        for B in BATCHES:
            for per in ROWS_PER_PATH:
                for nt in N_TIMES:
                    for K in N_STEPS:
                        cells = ['{}/{}'.format(query(lib.njode_workspace_bytes, ref, B, per * B, nt, K, f),
                                                query(lib.njode_plan_bytes, ref, B, per * B, nt, K, f))
                                 for f in FLAG_SETS]
                        print(name, budget, B, per * B, nt, K, *cells)


if __name__ == '__main__':
    if os.environ.get('NJODE_REC_BUDGET_GB') == TINY_BUDGET and '--child' in sys.argv:
        table(TINY_BUDGET)
    else:
        os.environ.pop('NJODE_REC_BUDGET_GB', None)
        table('default')
        sys.stdout.flush()
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), '--child'],
                                 env=dict(os.environ, NJODE_REC_BUDGET_GB=TINY_BUDGET)))
