"""
Host-side state of the Python call layer, on CPU tensors and hand-made plans, without the library:
who owns a workspace slot, which prefetched plan a call takes, what a deep copy starts with, where
the five pointers of a schedule struct point, and which files a training run writes when.
"""
import copy
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from njode_amd import _lib, models
from njode_amd.schedule import Schedule

NN = ((50, 'tanh'), (50, 'tanh'))
CPU = torch.device('cpu')


def _model(**opts):
    return models.NJODE(1, 10, 1, NN, NN, NN, use_rnn=False, bias=True, dropout_rate=0.1, options=opts)


def _call_with(slot):
    call = models._Call()
    call.ws_slot = slot
    return call


# -- 1. workspace pool ----------------------------------------------------------------------------
def test_workspace_slots_have_one_holder_at_a_time():
    m = _model()
    a = m._acquire_ws(1000, CPU)
    b = m._acquire_ws(1000, CPU)
    assert a is not b and a[1] and b[1]
    assert [id(s) for s in m._ws_pool] == [id(a), id(b)]
    assert a[0].numel() >= 1000 and a[0].dtype == torch.uint8

    call = _call_with(a)
    m._release_ws(call)
    assert not a[1] and call.ws_slot is None and b[1]
    m._release_ws(call)                       # (a second release is a no-op)
    assert not a[1] and b[1]
    assert m._acquire_ws(500, CPU) is a and a[1]     # a free slot that fits is taken again

    call = _call_with(a)
    del call                                  # the last reference to a call that holds a slot
    gc.collect()
    assert not a[1] and b[1]


def test_growth_drops_free_slots_that_are_too_small_and_no_taken_one():
    m = _model()
    a = m._acquire_ws(1000, CPU)
    b = m._acquire_ws(1000, CPU)
    m._release_ws(_call_with(a))
    big = m._acquire_ws(a[0].numel() + 1, CPU)
    assert big is not a and big is not b and big[1] and big[0].numel() > a[0].numel()
    assert [id(s) for s in m._ws_pool] == [id(b), id(big)]     # a (free, too small) went, b (taken) stayed


def test_no_slot_is_handed_out_while_taken():
    m = _model()
    rng = np.random.RandomState(0)
    held = []
    for _ in range(200):
        if held and rng.rand() < 0.45:
            m._release_ws(held.pop(rng.randint(len(held))))
            continue
        taken_before = [id(s) for s in m._ws_pool if s[1]]
        n = int(rng.choice([1, 700, 5000, 40000]))
        slot = m._acquire_ws(n, CPU)
        assert id(slot) not in taken_before and slot[1] and slot[0].numel() >= n
        assert any(s is slot for s in m._ws_pool)
        held.append(_call_with(slot))
        assert sorted(id(s) for s in m._ws_pool if s[1]) == sorted(id(c.ws_slot) for c in held)


# -- 2. plan matching -----------------------------------------------------------------------------
SIZES = (1, 3, 1, 2)
FLAGS = _lib.C_TRAIN | _lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_SCHED_KNOWN


def _batch_key():
    return torch.zeros(3, dtype=torch.int32), np.array([0, 3], dtype=np.int32)


def _plan(key, flags=FLAGS, sizes=SIZES):
    p = models._Plan()
    p.buf, p.done, p.flags, p.sizes, p.keep, p.pool = None, None, flags, sizes, [], None
    p.obs_idx, p.time_ptr, p.taken = key[0], key[1], False
    p.obs_version = key[0]._version
    p.pending, p.stream = False, None
    return p


def test_a_plan_is_found_by_identity_and_consumed_once():
    m = _model()
    key = _batch_key()
    twin = (key[0].clone(), key[1].copy())              # equal values, other objects
    p = _plan(key)
    m._plans.append(p)
    assert m._take_plan(None, twin, FLAGS, SIZES, False) is None
    assert m._take_plan(None, (key[0], twin[1]), FLAGS, SIZES, False) is None
    assert m._take_plan(None, (twin[0], key[1]), FLAGS, SIZES, False) is None
    assert m._plans == [p] and not p.taken
    assert m._take_plan(None, key, FLAGS, SIZES, False) is p
    assert m._plans == [] and p.taken
    with pytest.raises(RuntimeError, match='already consumed'):
        m._take_plan(p, key, FLAGS, SIZES, False)


def _bump(key):
    key[0].add_(1)


MISMATCHES = {
    'sizes': dict(sizes=(1, 3, 1, 3)),
    'flags': dict(flags=FLAGS | _lib.C_SCHED_TAIL),
    'version': dict(after=_bump),
    'want_hT': dict(want_hT=True),
}


@pytest.mark.parametrize('what', sorted(MISMATCHES))
def test_a_mismatched_plan_is_dropped_and_blocks_nobody(what):
    kw = MISMATCHES[what]
    m = _model()
    bad_key, good_key = _batch_key(), _batch_key()
    bad = _plan(bad_key, flags=kw.get('flags', FLAGS), sizes=kw.get('sizes', SIZES))
    good = _plan(good_key)
    m._plans.extend([bad, good])
    kw.get('after', lambda key: None)(bad_key)
    assert m._take_plan(None, bad_key, FLAGS, SIZES, kw.get('want_hT', False)) is None
    assert m._plans == [good]
    assert m._take_plan(None, good_key, FLAGS, SIZES, False) is good
    assert m._plans == []


def test_want_hT_is_met_by_the_tail_order_or_by_a_masked_model():
    key = _batch_key()
    m = _model()
    p = _plan(key, flags=FLAGS | _lib.C_NEED_HT)
    m._plans.append(p)
    assert m._take_plan(None, key, FLAGS, SIZES, True) is p
    masked = _model(masked=True, residual_enc_dec=False)
    p = _plan(key)
    assert masked._take_plan(p, None, FLAGS, SIZES, True) is p


def test_launch_only_flags_are_no_mismatch():
    m = _model()
    for extra in (_lib.C_LOSS_IN_BWD, _lib.C_PLAN_READY, _lib.C_ROWS_IN_FWD,
                  _lib.C_LOSS_IN_BWD | _lib.C_PLAN_READY | _lib.C_ROWS_IN_FWD):
        key = _batch_key()
        p = _plan(key)
        m._plans.append(p)
        assert m._take_plan(None, key, FLAGS | extra, SIZES, False) is p


# -- 3. deep copy ---------------------------------------------------------------------------------
RUNTIME_LISTS = ('_ws_pool', '_plans', '_deferred_slots')


def _used_model():
    m = _model()
    m.flat_parameters()
    m._acquire_ws(100, CPU)
    m._plans.append(_plan(_batch_key()))
    m._deferred_slots.append(3)
    return m


def test_a_deep_copy_starts_with_empty_pools_and_its_own_flat_vector():
    m = _used_model()
    c = copy.deepcopy(m)
    for name in RUNTIME_LISTS:
        assert getattr(c, name) == [] and getattr(c, name) is not getattr(m, name), name
        assert len(getattr(m, name)) == 1, name
    assert c._flat is None and c._flat_params is None and c._param_slices is None
    flat = c.flat_parameters()
    assert torch.equal(flat, m._flat)
    assert flat.data_ptr() != m._flat.data_ptr()
    base = flat.data_ptr()
    for (off, n, shape), p in zip(c._param_slices, c._flat_params):
        assert p.data_ptr() == base + 4 * off and tuple(p.shape) == tuple(shape)
    with torch.no_grad():
        flat.add_(1.0)
    assert not torch.equal(flat, m._flat)
    m._plans.clear()


def test_a_deep_copy_has_every_runtime_attribute_of_a_fresh_model():
    fresh, c = _model(), copy.deepcopy(_used_model())
    assert set(vars(fresh)) <= set(vars(c))
    assert '_deferred_stream' in vars(fresh) and c._deferred_stream is None
    assert not hasattr(fresh, '_last_stream')


# -- 4. schedule struct ---------------------------------------------------------------------------
def _read(addr, ctype, n):
    if n == 0:
        return np.zeros(0, dtype=np.dtype(ctype))
    return np.ctypeslib.as_array((ctype * n).from_address(addr)).copy()


@pytest.mark.parametrize('times,T,until_T,K,nt,tail,time_ptr', [
    ([], 0.05, False, 0, 0, False, [0]),
    ([], 0.05, True, 5, 0, True, [0]),
    ([0.02, 0.05], 0.1, True, 10, 2, True, [0, 2, 3]),
])
def test_schedule_struct_points_at_the_packed_arrays(times, T, until_T, K, nt, tail, time_ptr):
    s = Schedule(times, 0.01, T, until_T)
    assert (s.n_steps, s.n_times, s.has_tail()) == (K, nt, tail)
    time_ptr = np.asarray(time_ptr, dtype=np.int32)
    buf = np.full(s.packed_nbytes() // 4 + 16, -1, dtype=np.int32)    # (stands in for a pinned slot)
    assert s.pack_into(buf, time_ptr) == (K, nt)
    cs = s.struct(buf.ctypes.data)
    assert isinstance(cs, _lib.NjodeSchedule) and (cs.n_steps, cs.n_times) == (K, nt)
    base = buf.ctypes.data
    for p in (cs.step_dt, cs.step_t, cs.k_jump, cs.time_f32, cs.time_ptr):
        assert base <= (p or base) and (p or base) + 4 <= base + buf.nbytes
    np.testing.assert_array_equal(_read(cs.step_dt, ctypes.c_float, K), s.step_dt)
    np.testing.assert_array_equal(_read(cs.step_t, ctypes.c_float, K), s.step_t)
    np.testing.assert_array_equal(_read(cs.k_jump, ctypes.c_int32, nt), s.k_jump)
    np.testing.assert_array_equal(_read(cs.time_f32, ctypes.c_float, nt), s.time_f32)
    np.testing.assert_array_equal(_read(cs.time_ptr, ctypes.c_int32, nt + 1), time_ptr)
    assert (buf[2 * K + 3 * nt + 1:] == -1).all()
    if K:
        assert s.step_dt.dtype == np.float32 and abs(float(s.step_dt.sum()) - T) < 1e-6


# -- 5. run bookkeeping ---------------------------------------------------------------------------
COLUMNS = ['epoch', 'train_time', 'eval_time', 'train_loss', 'eval_loss', 'eval_metric', 'eval_metric_2']
# the followed column improves on epochs 1 and 3 only (epoch 5 ties the best: no improvement); the
# other one improves every epoch, so following the wrong column writes a best checkpoint every epoch
FOLLOWED = [5.0, 6.0, 4.0, 4.5, 4.0]
OTHER = [1.0, 0.9, 0.8, 0.7, 0.6]
# (parent's train.train: eval_loss, column 4; ``last_checkpoint`` + metric file every ``save_every``
# epochs AND on improvement.  Parent's record loops: eval_metric, column 5; ``last_checkpoint`` +
# metric file every ``save_every`` epochs only.  Both: ``best_checkpoint`` on improvement.)
POLICIES = {
    'train': dict(best_col=4, save_on_best=True, last=[1, 2, 3, 4, 4], best=[1, 1, 3, 3, 3],
                  rows_on_disk=[1, 2, 3, 4, 4]),
    'records': dict(best_col=5, save_on_best=False, last=[None, 2, 2, 4, 4], best=[1, 1, 3, 3, 3],
                    rows_on_disk=[None, 2, 2, 4, 4]),
}


def _row(epoch, best_col):
    row = [epoch, 0.5, 0.25, 2.0, 0.0, 0.0, 7.0]
    row[best_col], row[9 - best_col] = FOLLOWED[epoch - 1], OTHER[epoch - 1]
    return row


def _csv_text(rows):
    lines = [',' + ','.join(COLUMNS)] + ['{},'.format(i) + ','.join(repr(x) for x in r)
                                         for i, r in enumerate(rows)]
    return ''.join(l + '\r\n' for l in lines)


def _ckpt_epoch(path):
    f = os.path.join(path, 'checkpt.tar')
    return torch.load(f, weights_only=False)['epoch'] if os.path.exists(f) else None


@pytest.mark.parametrize('policy', sorted(POLICIES))
def test_run_files_follow_the_policy(policy, tmp_path):
    from njode_amd.run import Run
    pol = POLICIES[policy]
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0005)
    logged = []
    run = Run(str(tmp_path), 7, COLUMNS, logged.append, pol['best_col'], pol['save_on_best'])
    run.resume(model, opt, CPU, True, False)          # nothing to resume from: a no-op
    assert model.epoch == 1 and run.saved_rows == []
    model_dir = os.path.join(str(tmp_path), 'id-7')
    metric_file = os.path.join(model_dir, 'metric_id-7.csv')
    rows = [_row(e, pol['best_col']) for e in range(1, 6)]
    for e in range(1, 6):
        model.epoch = e
        if policy == 'train':       # (each loop's own order of the two calls)
            run.end_of_epoch(model, opt, rows[e - 1], 2)
            run.new_best(model, opt, rows[e - 1][pol['best_col']])
        else:
            run.new_best(model, opt, rows[e - 1][pol['best_col']])
            run.end_of_epoch(model, opt, rows[e - 1], 2)
        assert _ckpt_epoch(os.path.join(model_dir, 'last_checkpoint')) == pol['last'][e - 1], e
        assert _ckpt_epoch(os.path.join(model_dir, 'best_checkpoint')) == pol['best'][e - 1], e
        n = pol['rows_on_disk'][e - 1]
        if n is None:
            assert not os.path.exists(metric_file)
        else:
            with open(metric_file, newline='') as f:
                assert f.read() == _csv_text(rows[:n]), e
    assert len(logged) == 2 and all('save new best model' in s for s in logged)
    assert run.best == 4.0 and run.pending == [rows[4]]
    assert sorted(os.listdir(model_dir)) == ['best_checkpoint', 'last_checkpoint', 'metric_id-7.csv']

    model2 = _model()
    opt2 = torch.optim.Adam(model2.parameters(), lr=1e-3, weight_decay=0.0005)
    run2 = Run(str(tmp_path), 7, COLUMNS, logged.append, pol['best_col'], pol['save_on_best'])
    run2.resume(model2, opt2, CPU, True, False)
    assert run2.saved_rows == [[float(x) for x in r] for r in rows[:4]]
    assert run2.best == 4.0           # min of the followed column (the other one's is 0.7)
    assert model2.epoch == 4 + 1
    for k, v in model.state_dict().items():
        assert torch.equal(model2.state_dict()[k], v), k

    run3 = Run(None, 7, COLUMNS, logged.append, pol['best_col'], pol['save_on_best'])
    run3.new_best(model, opt, 0.0)
    run3.end_of_epoch(model, opt, rows[0], 1)
    assert run3.pending == [rows[0]] and run3.saved_rows == [] and len(logged) == 2
