"""Online filtering on the shape-generic kernels, the part that needs no GPU: exported symbols, the
verdict on a list of shapes against the Python restatement of ``build_model``
(``gen_envelope.restate``), the argument checks of the new entry points from pointers that are never
followed, and the ``kernels=`` keyword of ``NJODE.online``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gen_envelope
import online_gen_util as ogu
import online_util
from njode_amd import _lib, models
from njode_amd.build import CONFIGS
from test_online_host import dims_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('njode_online_gen_supported', 'njode_online_tables_bytes', 'njode_online_tables_f32',
       'njode_online_gen_reset_f32', 'njode_online_gen_advance_f32', 'njode_online_gen_observe_f32',
       'njode_online_gen_predict_f32')


def test_symbols_declared_listed_and_exported():
    header = open(os.path.join(REPO, 'include', 'njode_online.h')).read()
    declared = set(re.findall(r'\b(njode_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name


def _verdict(raw):
    L = _lib.lib()
    ok = L.njode_online_gen_supported(ctypes.byref(gen_envelope.dims_of(*raw)))
    return ok, L.njode_last_error().decode()


@pytest.mark.parametrize('name', sorted(ogu.SHAPES))
def test_accepted_shapes(name):
    raw = ogu.raw_of_cfg(ogu.SHAPES[name])
    why, model = gen_envelope.restate(*raw)
    assert why is None, (name, why)
    ok, msg = _verdict(raw)
    assert ok == 1, (name, msg)
    assert msg.startswith('online: ') and len(msg) > 12, msg
    # the same verdict on the description the Python model hands over
    m = models.NJODE(**ogu.SHAPES[name]).eval()
    assert _lib.lib().njode_online_gen_supported(ctypes.byref(m._get_dims())) == 1


@pytest.mark.parametrize('i', range(len(CONFIGS)))
def test_every_build_table_shape_is_accepted(i):
    L = _lib.lib()
    raw = ogu.raw_of_cfg(online_util.model_cfg(CONFIGS[i]))
    assert gen_envelope.restate(*raw)[0] is None
    assert L.njode_online_gen_supported(ctypes.byref(dims_of(CONFIGS[i]))) == 1, L.njode_last_error()
    assert L.njode_last_error().decode().startswith('online: ')


@pytest.mark.parametrize('name', sorted(ogu.REFUSED))
def test_refused_shapes(name):
    raw = ogu.REFUSED[name]
    why, _ = gen_envelope.restate(*raw)
    assert why is not None, name
    ok, msg = _verdict(raw)
    assert ok == 0, (name, msg)
    assert msg.startswith('online: ' + why) or (msg.startswith('online: ') and why in msg), (msg, why)
    # ... and every entry point says NJODE_E_UNSUPPORTED with the same reason
    L = _lib.lib()
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    d = gen_envelope.dims_of(*raw)
    assert L.njode_online_gen_reset_f32(ctypes.byref(d), 256, 256, 1 << 30, ctypes.byref(st), None, 2, 256, 0,
                                        None) == _lib.E_UNSUPPORTED
    assert L.njode_last_error().decode() == msg
    out = ctypes.c_size_t(0)
    assert L.njode_online_tables_bytes(ctypes.byref(d), ctypes.byref(out)) == _lib.E_UNSUPPORTED


def test_reasons_name_the_cause():
    assert gen_envelope.R_LDS in _verdict(ogu.REFUSED['lds_overflow'])[1]
    assert gen_envelope.R_RNN in _verdict(ogu.REFUSED['rnn_4h_above_1024'])[1]
    assert gen_envelope.R_MASKED in _verdict(ogu.REFUSED['masked_d_ne_dout'])[1]
    assert gen_envelope.R_RESIDUAL in _verdict(ogu.REFUSED['residual_mismatch'])[1]
    assert _lib.lib().njode_online_gen_supported(None) == 0


def test_the_clock_arrays_count_against_the_lds_limit():
    """The one verdict of this family's own: build_model accepts the shape, the restatement too, and
    the per-chain clocks behind the LDS images no longer fit."""
    raw = ogu.LDS_WINDOW
    why, model = gen_envelope.restate(*raw)
    assert why is None and gen_envelope.LDS_LIMIT - 576 < model['lds_bytes'] <= gen_envelope.LDS_LIMIT
    L = _lib.lib()
    d = gen_envelope.dims_of(*raw)
    assert L.njode_supported(ctypes.byref(d)) == 1
    ok, msg = _verdict(raw)
    assert ok == 0 and msg.startswith('online: ') and 'per-chain clocks' in msg, msg
    out = ctypes.c_size_t(0)
    assert L.njode_online_tables_bytes(ctypes.byref(d), ctypes.byref(out)) == _lib.E_UNSUPPORTED
    # one unit of hidden size less and it fits
    smaller = (raw[0], raw[1] - 1) + raw[2:]
    assert gen_envelope.restate(*smaller)[1]['lds_bytes'] + 576 <= gen_envelope.LDS_LIMIT
    assert _verdict(smaller)[0] == 1


def _tables_bytes(d):
    out = ctypes.c_size_t(0)
    assert _lib.lib().njode_online_tables_bytes(ctypes.byref(d), ctypes.byref(out)) == _lib.NJODE_OK
    return int(out.value)


def test_tables_bytes():
    for name in ('w80', 'gru_w80', 'climate_w400_h50', 'none_h100'):
        raw = ogu.raw_of_cfg(ogu.SHAPES[name])
        nbytes = _tables_bytes(gen_envelope.dims_of(*raw))
        # at least the forward tables of every layer: [output tile][k-step][64 lanes] floats
        _, model = gen_envelope.restate(*raw)
        fwd = sum(L['MT'] * L['Qp'] * 64 for L in model['layers']) * 4
        assert nbytes > fwd > 0 and nbytes % 4 == 0, (name, nbytes, fwd)
    d = gen_envelope.dims_of(*ogu.raw_of_cfg(ogu.SHAPES['w80']))
    assert _lib.lib().njode_online_tables_bytes(ctypes.byref(d), None) == _lib.E_BADARG


def _calls(L, d, st, tables, tb, spt, delta_t=0.1, max_steps=5, n=2, M=None, only=(0, 1, 2, 3)):
    """The modes ``only`` (reset, advance, observe, predict), every pointer a value that must not be
    followed: list a mode only where the arguments make it refuse."""
    f = [lambda: L.njode_online_gen_reset_f32(ctypes.byref(d), 256, tables, tb, ctypes.byref(st), None, n, 256, spt,
                                              None),
         lambda: L.njode_online_gen_advance_f32(ctypes.byref(d), 256, tables, tb, ctypes.byref(st), None, n, 256,
                                                delta_t, max_steps, spt, 256, None),
         lambda: L.njode_online_gen_observe_f32(ctypes.byref(d), 256, tables, tb, ctypes.byref(st), None, n, 256, 256,
                                                M, delta_t, max_steps, spt, None, None, 256, None),
         lambda: L.njode_online_gen_predict_f32(ctypes.byref(d), 256, tables, tb, ctypes.byref(st), None, n, 256, 3,
                                                delta_t, max_steps, spt, 256, 256, None)]
    return [f[i]() for i in only]


def test_entry_points_refuse_before_any_launch():
    L = _lib.lib()
    d = gen_envelope.dims_of(*ogu.raw_of_cfg(ogu.SHAPES['w80']))
    tb = _tables_bytes(d)
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    # tables: null, one byte short
    assert _calls(L, d, st, None, tb, 0) == [_lib.E_BADARG] * 4
    assert 'tables' in L.njode_last_error().decode()
    assert _calls(L, d, st, 256, tb - 1, 0) == [_lib.E_BADARG] * 4
    assert 'tables_bytes' in L.njode_last_error().decode()
    assert L.njode_online_tables_f32(ctypes.byref(d), 256, 256, tb - 1, None) == _lib.E_BADARG
    assert L.njode_online_tables_f32(ctypes.byref(d), 256, None, tb, None) == _lib.E_BADARG
    assert L.njode_online_tables_f32(ctypes.byref(d), None, 256, tb, None) == _lib.E_BADARG
    # series_per_tile
    for spt in (-1, 3, 5, 12, 32, 17):
        assert _calls(L, d, st, 256, tb, spt) == [_lib.E_BADARG] * 4, spt
        assert 'series_per_tile' in L.njode_last_error().decode()
    # the bad-clock cases of the wave family's test (reset takes no clock)
    for delta_t, max_steps in ((0.0, 5), (-1.0, 5), (float('inf'), 5), (float('nan'), 5), (0.1, 0), (0.1, -3)):
        rcs = _calls(L, d, st, 256, tb, 0, delta_t, max_steps, only=(1, 2, 3))
        assert rcs == [_lib.E_BADARG] * 3, (delta_t, max_steps)
    # M on an unmasked model, a missing M on a masked one, more rows than series without ids, Q <= 0
    assert _calls(L, d, st, 256, tb, 0, M=256, only=(2,)) == [_lib.E_BADARG]
    dm = gen_envelope.dims_of(*ogu.raw_of_cfg(ogu.SHAPES['climate_w400_h50']))
    assert _calls(L, dm, st, 256, _tables_bytes(dm), 0, only=(2,)) == [_lib.E_BADARG]
    assert 'needs M' in L.njode_last_error().decode()
    assert _calls(L, d, st, 256, tb, 0, n=5) == [_lib.E_BADARG] * 4
    assert _calls(L, d, st, 256, tb, 0, n=-1) == [_lib.E_BADARG] * 4
    assert L.njode_online_gen_predict_f32(ctypes.byref(d), 256, 256, tb, ctypes.byref(st), None, 2, 256, 0, 0.1, 5, 0,
                                          256, 256, None) == _lib.E_BADARG
    # null state array, null params, null dims
    bad = _lib.NjodeOnlineState(256, None, 768, 1024, 4)
    assert _calls(L, d, bad, 256, tb, 0) == [_lib.E_BADARG] * 4
    assert L.njode_online_gen_reset_f32(ctypes.byref(d), None, 256, tb, ctypes.byref(st), None, 2, 256, 0,
                                        None) == _lib.E_BADARG
    assert L.njode_online_gen_reset_f32(None, 256, 256, tb, ctypes.byref(st), None, 2, 256, 0, None) == _lib.E_BADARG
    # n == 0: nothing is launched (no device here to launch on)
    assert _calls(L, d, st, 256, tb, 16, n=0) == [_lib.NJODE_OK] * 4


# ---- the Python layer -------------------------------------------------------------------------------
def test_kernels_keyword():
    demo = models.NJODE(**online_util.model_cfg(CONFIGS[online_util.DEMO])).eval()
    for bad in ('x', '', None, 'Wave'):
        with pytest.raises(ValueError, match='kernels'):
            demo.online(4, 0.01, kernels=bad)
    assert demo.online(4, 0.01).kernels == 'wave'
    assert demo.online(4, 0.01, kernels='auto').kernels == 'wave'
    assert demo.online(4, 0.01, kernels='generic').kernels == 'generic'
    for i in online_util.REFUSED:
        m = models.NJODE(**online_util.model_cfg(CONFIGS[i])).eval()
        assert m.online(4, 0.01, kernels='auto').kernels == 'generic'
    w80 = models.NJODE(**ogu.SHAPES['w80']).eval()
    st = w80.online(4, 0.01, kernels='auto')
    assert st.kernels == 'generic' and st.series_per_tile is None
    # construction launches nothing: a CPU model constructs, and a call names the device
    assert st._tables is None and st.h.device.type == 'cpu'
    with pytest.raises(RuntimeError, match='no CPU path'):
        st.reset(torch.zeros(4, 1))


@pytest.mark.parametrize('name', ['w80', 'gru_w80'] + ['cfg{}'.format(i) for i in online_util.REFUSED])
def test_default_refusal_quotes_the_reason_and_names_generic(name):
    cfg = ogu.SHAPES.get(name) or online_util.model_cfg(CONFIGS[int(name[3:])])
    m = models.NJODE(**cfg).eval()
    with pytest.raises(NotImplementedError) as e:
        m.online(4, 0.01)
    _lib.lib().njode_online_supported(ctypes.byref(m._get_dims()))
    assert _lib.lib().njode_last_error().decode() in str(e.value)
    assert "kernels='generic'" in str(e.value)


def test_generic_refusal_carries_the_library_reason():
    class Dims:      # a model whose description the generic family refuses (4 H > 1024 with use_rnn)
        training = False

        def _get_dims(self):
            return gen_envelope.dims_of(*ogu.REFUSED['rnn_4h_above_1024'])
    from njode_amd.online import OnlineState
    for kernels in ('generic', 'auto'):
        with pytest.raises(NotImplementedError, match='use_rnn'):
            OnlineState(Dims(), 4, 0.01, kernels=kernels)
    with pytest.raises(NotImplementedError) as e:
        OnlineState(Dims(), 4, 0.01)
    assert "kernels='generic'" not in str(e.value)      # no hint where the other family refuses too


@pytest.fixture(scope='module')
def states():
    """An unmasked and a masked generic state on the CPU: every check fires before the device is asked for."""
    return {'demo': (models.NJODE(**ogu.SHAPES['one_layer_easy']).eval().online(5, 0.01, kernels='generic'), 2),
            'masked': (models.NJODE(**ogu.SHAPES['climate_w400_h50']).eval().online(5, 0.01, kernels='generic'), 5)}


def test_value_errors_on_a_generic_state(states):
    """test_online_host.test_value_errors, on states of the generic family."""
    import test_online_host
    test_online_host.test_value_errors(states)
    st, d = states['demo']
    st.model.train()
    try:
        with pytest.raises(ValueError, match='eval'):
            st.advance([0.1], ids=[0])
    finally:
        st.model.eval()


def test_series_per_tile_is_checked_on_the_host(states):
    st, d = states['demo']
    assert st.series_per_tile is None and st._spt() == 0
    try:
        for bad in (3, 0, 32, -1):
            st.series_per_tile = bad
            with pytest.raises(ValueError, match='series_per_tile'):
                st._spt()
        st.series_per_tile = 8
        assert st._spt() == 8
    finally:
        st.series_per_tile = None


def test_tables_stamp_sees_parameter_writes():
    """What ``_ensure_tables`` compares changes under load_state_dict and under an in-place update."""
    m = models.NJODE(**ogu.SHAPES['w80']).eval()
    assert m.online(3, 0.01, kernels='generic')._tables_stamp is None
    m._ensure_flat(full=True)

    def stamp():
        m._ensure_flat(full=True)
        return (m._flat.data_ptr(), m._flat._version, m._param_writes) + tuple(p._version for p in m._flat_params)
    s0 = stamp()
    assert stamp() == s0
    m.load_state_dict({k: v + 0.5 for k, v in m.state_dict().items()})
    s1 = stamp()
    assert s1 != s0
    with torch.no_grad():
        next(m.parameters()).add_(1.0)
    assert stamp() != s1
    assert np.isfinite(m._flat.numpy()).all()
