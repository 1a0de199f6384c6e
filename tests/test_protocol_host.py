"""Host side of the device evaluation protocols (include/njode_protocol.h, njode_amd/protocol.py,
``physionet_eval.evaluate_model_device``, ``climate_eval.evaluate_model_device``): what is
declared, exported and built, the stated workspace size, and the refusals that come before any
launch.  No GPU is needed: the model handed to the routes raises as soon as it is called."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from njode_amd import _lib, build, climate_eval, physionet_eval

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('njode_protocol_bytes', 'njode_protocol_rows', 'njode_protocol_score_f32')

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason='libnjode_hip.so not built in this checkout (run __graft_entry__.build())')


def test_header_exports_and_build_list():
    header = open(os.path.join(REPO, 'include', 'njode_protocol.h')).read()
    declared = set(re.findall(r'\bint (njode_[a-z0-9_]+)\s*\(', header))
    assert declared == set(NAMES)
    for macro in ('NJODE_ROWS_CLOSEST 0', 'NJODE_ROWS_FIRST_NEAREST 1'):
        assert '#define ' + macro in header
    assert set(NAMES) <= set(_lib.EXPORTS)
    assert (_lib.ROWS_CLOSEST, _lib.ROWS_FIRST_NEAREST) == (0, 1)
    src = open(build.__file__).read()
    assert 'njode_protocol.hip' in src and os.path.exists(os.path.join(build.CSRC, 'njode_protocol.hip'))
    # compiled like the producer: no contraction
    line = next(l for l in src.splitlines() if 'njode_protocol.hip' in l and 'cmd' in l)
    assert '-ffp-contract=off' in line
    # the job struct of the header, field for field
    body = header.split('typedef struct NjodeProtocolJob {')[1].split('} NjodeProtocolJob;')[0]
    fields = re.findall(r'(\w+);', body)
    assert fields == [f[0] for f in _lib.NjodeProtocolJob._fields_]


@needs_lib
def test_library_exports():
    L = _lib.lib()
    for sym in NAMES:
        assert hasattr(L, sym), sym


def _bytes(n_rows, n_query, B, dim):
    need = ctypes.c_size_t(0)
    rc = _lib.lib().njode_protocol_bytes(n_rows, n_query, B, dim, ctypes.byref(need))
    return rc, need.value


@needs_lib
def test_stated_workspace_is_monotone_and_refuses_negative_sizes():
    base = dict(n_rows=300, n_query=130, B=50, dim=41)
    grids = {'n_rows': (0, 1, 2, 300, 3000, 100000),
             'n_query': (0, 1, 2, 5, 6, 7, 63, 130, 131, 257, 1025, 1500, 40000),
             'B': (1, 2, 6, 49, 50, 51, 511, 512, 513, 800, 1023, 1024, 1025, 4000),
             'dim': (1, 2, 5, 41, 63, 64, 65, 128, 129, 255, 256, 257, 300, 512)}
    for name, values in grids.items():
        sizes = []
        for v in values:
            rc, n = _bytes(**dict(base, **{name: v}))
            assert rc == 0, (name, v)
            assert n > 0 and n % 256 == 0
            sizes.append(n)
        assert sizes == sorted(sizes), (name, sizes)
    # a second, small corner of the table: every neighbour of every point
    pts = (1, 2, 3, 7, 50)
    for q in pts:
        for B in pts:
            for d in pts:
                here = _bytes(10, q, B, d)[1]
                assert _bytes(10, q + 1, B, d)[1] >= here
                assert _bytes(10, q, B + 1, d)[1] >= here
                assert _bytes(10, q, B, d + 1)[1] >= here
    for name in base:
        rc, _ = _bytes(**dict(base, **{name: -1}))
        assert rc == _lib.E_BADARG, name
        assert _lib.lib().njode_last_error()
    assert _bytes(10, 5, 0, 3)[0] == _lib.E_BADARG and _bytes(10, 5, 3, 0)[0] == _lib.E_BADARG
    assert _lib.lib().njode_protocol_bytes(10, 5, 3, 3, None) == _lib.E_BADARG


# ---- refusals of the Python routes, before any launch -------------------------------------------
class _NeverCalled:
    """A model that fails the test if the route gets as far as calling it."""

    def eval(self):
        pass

    def __call__(self, *a, **kw):
        raise AssertionError('the model was called: the refusal came too late')


def _physio():
    return physionet_eval.make_eval_batch(batch_size=6, n_grid=240, n_obs_range=(6, 16), seed=3)


def _climate():
    return climate_eval.make_climate_batch(batch_size=7, T=20, T_val=15, n_obs_range=(5, 12), seed=1)


def test_physionet_route_refuses_before_any_launch():
    b = _physio()
    dt, T = b['delta_t'], b['T']
    run = lambda bb, device='cuda': physionet_eval.evaluate_model_device(_NeverCalled(), [bb], device, dt, T)
    with pytest.raises(ValueError):
        run(b, 'cpu')
    # the range check of get_comparison_times_ind, word for word
    from njode_amd.schedule import Schedule
    path_t = Schedule(b['times'], dt, T, True).path_t
    for times_val in (np.concatenate([[0.0], b['times_val'][1:]]),            # not after the start
                      np.concatenate([b['times_val'][:-1], [T + 0.5]])):       # beyond the path
        with pytest.raises(AssertionError) as host:
            physionet_eval.get_comparison_times_ind(path_t, times_val)
        with pytest.raises(AssertionError) as dev:
            run(dict(b, times_val=times_val))
        assert str(dev.value) == str(host.value) and str(host.value).startswith('mins: ')
    with pytest.raises(ValueError):
        run(dict(b, vals_val=b['vals_val'][:-1]))                              # B
    with pytest.raises(ValueError):
        run(dict(b, mask_val=b['mask_val'][:, :, :-1]))                        # dim
    with pytest.raises(ValueError):
        run(dict(b, times_val=b['times_val'][:-1]))                            # each other
    with pytest.raises(ValueError):
        run(dict(b, vals_val=b['vals_val'][:, :-1]))
    # the second batch is checked before the first is run
    with pytest.raises(ValueError):
        physionet_eval.evaluate_model_device(_NeverCalled(), [b, dict(b, vals_val=b['vals_val'][:-1])],
                                             'cuda', dt, T)


def test_climate_route_refuses_before_any_launch():
    b = _climate()
    dt, T = b['delta_t'], b['T']
    run = lambda bb, device='cuda': climate_eval.evaluate_model_device(_NeverCalled(), [bb], device, dt, T)
    with pytest.raises(ValueError):
        run(b, 'cpu')
    bad = b['index_val'].copy()
    bad[0] = 7                                                                 # B = 7
    with pytest.raises(ValueError):
        run(dict(b, index_val=bad))
    bad = b['index_val'].copy()
    bad[-1] = -1
    with pytest.raises(ValueError):
        run(dict(b, index_val=bad))
    with pytest.raises(ValueError):
        run(dict(b, index_val=b['index_val'].astype(np.float64)))
    with pytest.raises(ValueError):
        run(dict(b, index_val=b['index_val'][:-1]))
    with pytest.raises(ValueError):
        run(dict(b, X_val=b['X_val'][:-1]))
    with pytest.raises(ValueError):
        run(dict(b, M_val=b['M_val'][:, :-1]))
    with pytest.raises(ValueError):
        run(dict(b, times_val=b['times_val'][:-1]))


def test_wrappers_refuse_cpu_tensors_and_mixed_layouts():
    from njode_amd import protocol
    pred = torch.zeros(5, 2, 3)
    rows = torch.zeros(4, dtype=torch.int32)
    vals = torch.zeros(2, 4, 3)
    with pytest.raises(ValueError):
        protocol.rows(torch.zeros(5, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), 'closest')
    with pytest.raises(ValueError):
        protocol.rows(torch.zeros(5, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), 'nearest')
    with pytest.raises(ValueError):
        protocol.score(pred, rows, vals=vals, mask=vals)                       # CPU tensors
    with pytest.raises(ValueError):
        protocol.score(pred, rows)                                             # neither layout
    with pytest.raises(ValueError):
        protocol.score(pred, rows, vals=vals, mask=vals, X_val=torch.zeros(4, 3))   # both
    with pytest.raises(ValueError):
        protocol.score(pred, rows, vals=vals)                                  # half of one
