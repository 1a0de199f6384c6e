"""The PhysioNet and climate evaluation protocols on the GPU (C ABI include/njode_protocol.h;
``njode_amd.protocol``, ``physionet_eval.evaluate_model_device``,
``climate_eval.evaluate_model_device``) against the host routes, which stay the yardstick.

What is held to what (u = 2**-53, the unit roundoff of float64):

* **Rows.**  ``protocol.rows(..., 'closest')`` equals ``get_comparison_times_ind`` integer for
  integer; ``'first_nearest'`` selects the rows ``extract_from_path`` selects: the predictions
  gathered from a ``path_y`` whose entries are all distinct are equal bit for bit.
* **n_obs** is exact (a float64 sum of small integers).
* **sq_sum.**  The expected value is numpy's float64 sum of the host's fp32 terms
  ``((pred - val) ** 2) * mask``; the kernel forms the same fp32 terms (no contraction) and sums
  them in float64 in another order.  All terms are non-negative, so any order of the N - 1
  additions of N terms stays within ``(N - 1) u`` relative of the exact sum: that is the
  allowance (the form ``tests/test_hip_cond_exp.py`` uses for the fused metric).
* **attr_mse.**  Both sides form ``(float64(pred) - float64(val)) ** 2`` -- the same two IEEE
  operations, equal bits -- so only the order of the sums differs.  The longest chain of one
  result: T2 terms of one (path, attribute) summed (T2 - 1 roundings), one division by the count
  (1), ``dim`` quotients summed (dim - 1) and divided by ``dim`` (1), ``B`` means summed (B - 1)
  and divided by ``B`` (1): T2 + dim + B roundings of non-negative quantities, each within ``u``
  relative, hence an allowance of ``(T2 + dim + B) u`` relative.
  Largest observed error / allowance on the MI355X (``WORST``, printed by the dense and sparse
  tests): 4.2e-5 for ``sq_sum`` (B = 50, T2 = 130, dim = 5) and 0.084 for ``attr_mse`` (B = 6,
  T2 = 1, dim = 5); also recorded in DESIGN section 4e.
* **accumulate** adds a call's finished sums once: two batches into one ``out`` equal the float64
  sum of two separate calls to the last bit.  Two calls give equal bits.
* **Stated sizes.**  ``out``, ``rows`` and the workspace sit at exactly their stated byte counts
  between bands of a pattern that must survive; a workspace one byte short is refused.
* **End to end** on the ``g8`` goldens' models: ``loss_val`` equal to the host route's (the same
  forward); ``mse_val`` / ``mse_val_2`` within rel 1e-5 of it (the host sums fewer than 2**20
  non-negative fp32 terms pairwise, blocks of 128 in eight accumulators: under about
  40 * 2**-24 = 2.4e-6 relative; ``mse_val_2`` adds two fp32 means; the device sums in float64);
  against the goldens with the host route's own tolerances (``LOSS_RTOL``, 1e-4).
"""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import Golden
from hip_util import LOSS_RTOL, hip_model
from njode_amd import _lib, climate_eval, physionet_eval, protocol
from njode_amd.schedule import Schedule

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DEV = 'cuda'
WORST = {}


def _record(what, err, allow):
    if allow > 0:
        WORST[what] = max(WORST.get(what, 0.0), err / allow)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_rows(path_t, query, rule):
    got = protocol.rows(_dev(np.asarray(path_t, dtype=np.float64)), _dev(np.asarray(query, dtype=np.float64)), rule)
    assert got.dtype == torch.int32 and got.is_cuda
    return got.cpu().numpy().astype(np.int64)


def first_nearest_on_host(t_vec, query):
    """rows of ``extract_from_path``, read off a path_y that holds its own row number"""
    y = np.arange(len(t_vec), dtype=np.float32).reshape(-1, 1, 1)
    got = climate_eval.extract_from_path(t_vec, y, query, np.zeros(len(query), dtype=np.int64))
    return got.reshape(-1).astype(np.int64)


# ---- rows -------------------------------------------------------------------------------------------
def test_rows_of_the_goldens():
    g = Golden('g8_physionet_eval')
    for i in range(int(g['n_batches'])):
        p = 'b{}/'.format(i)
        got = dev_rows(g[p + 'path_t'], g[p + 'times_val'], 'closest')
        assert np.array_equal(got, g[p + 'cmp_ind'])
        assert np.array_equal(got, physionet_eval.get_comparison_times_ind(g[p + 'path_t'], g[p + 'times_val']))
    g = Golden('g8_climate_eval')
    for i in range(int(g['n_batches'])):
        p = 'b{}/'.format(i)
        path_t, B = g[p + 'path_t'], int(g[p + 'batch_size'])
        t_vec = np.around(path_t, 1).astype(np.float32)
        # every entry distinct (and exact in fp32): equal bits = the same row and station
        path_y = np.arange(len(path_t) * B * 5, dtype=np.float32).reshape(len(path_t), B, 5)
        want = climate_eval.extract_from_path(t_vec, path_y, g[p + 'times_val'], g[p + 'index_val'])
        rows = dev_rows(t_vec.astype(np.float64), g[p + 'times_val'], 'first_nearest')
        got = path_y[rows, g[p + 'index_val']]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rows_hand_made_vectors():
    t = np.array([0.0, 0.1, 0.1, 0.2, 0.4])
    assert dev_rows(t, [0.1, 0.15, 0.16, 0.31, 0.4], 'closest').tolist() == [1, 2, 3, 4, 4]
    t32 = np.array([0.0, 0.125, 0.125, 0.25, 0.5], dtype=np.float32)
    q = np.array([0.125, 0.2, 0.375, 0.38, 0.9])
    assert dev_rows(t32.astype(np.float64), q, 'first_nearest').tolist() == [1, 3, 3, 4, 4] == \
        first_nearest_on_host(t32, q).tolist()
    # two rows
    two = np.array([0.0, 1.0])
    q = np.array([1e-3, 0.5 - 1e-9, 0.5, 0.5 + 1e-9, 1.0 - 5e-11, 1.0, 1.0 + 5e-11])
    assert np.array_equal(dev_rows(two, q, 'closest'), physionet_eval.get_comparison_times_ind(two, q))
    assert dev_rows(two, q, 'closest').tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(dev_rows(two, q, 'first_nearest'), first_nearest_on_host(two.astype(np.float32), q))
    # a single row answers everything
    assert dev_rows(np.array([0.25]), [0.0, 0.25, 7.0], 'first_nearest').tolist() == [0, 0, 0]
    assert dev_rows(np.array([0.25]), [0.0, 0.25, 7.0], 'closest').tolist() == [0, 0, 0]


def _edge_queries(path_t):
    """on every time, 5e-11 and 2e-10 to either side of it, every exact midpoint, the last
    interval, the last time and just past it"""
    q = []
    for v in np.unique(path_t):
        q += [v, v - 5e-11, v + 5e-11, v - 2e-10, v + 2e-10]
    u = np.unique(path_t)
    q += list(0.5 * (u[:-1] + u[1:]))
    q += [u[-2] + 0.75 * (u[-1] - u[-2]), u[-1], u[-1] + 5e-11]
    return np.array(q)


def test_rows_repeated_times_windows_ties_and_the_clamp():
    # binary fractions: the midpoints are exact ties; times repeat twice and three times
    path_t = np.array([0.0, 0.125, 0.25, 0.25, 0.375, 0.5, 0.5, 0.5, 0.625, 0.75, 0.75, 1.0])
    q = _edge_queries(path_t)
    ok = (q > path_t.min()) & (q < path_t.max() + 1e-10)           # what the host function accepts
    want = physionet_eval.get_comparison_times_ind(path_t, q[ok])
    got = dev_rows(path_t, q, 'closest')
    assert np.array_equal(got[ok], want)
    # (ties go left, 1e-10 window, first interval of a repeated time, clamp -- spelled out)
    n = len(path_t)
    assert dev_rows(path_t, [0.1875, 0.25, 0.25 + 5e-11, 0.25 - 5e-11, 0.25 + 2e-10, 0.25 - 2e-10, 0.5, 0.875,
                             0.9, 1.0, 1.0 + 5e-11], 'closest').tolist() == [1, 2, 2, 2, 3, 2, 5, 10, 11, 11, 11]
    # past the path: the clamp (the host function asserts there; the rule says n_rows - 1)
    assert dev_rows(path_t, [1.0 + 2e-10, 1.5, 1e9], 'closest').tolist() == [n - 1] * 3
    assert dev_rows(path_t, [0.0, -1.0], 'closest').tolist() == [0, n - 1]   # the rule, literally
    # the climate rule on the same path (exact in fp32), queries before, on, between and past
    q2 = np.concatenate([q, [-3.0, 1.5, 1e9]])
    assert np.array_equal(dev_rows(path_t, q2, 'first_nearest'),
                          first_nearest_on_host(path_t.astype(np.float32), q2))
    assert dev_rows(path_t, [0.25, 0.3125, 0.5, 0.5625, 0.75, 0.874, 0.876, 2.0],
                    'first_nearest').tolist() == [2, 2, 5, 5, 9, 9, 11, 11]


@pytest.mark.parametrize('n_query', [1, 63, 257, 1025])
def test_rows_many_queries(n_query):
    rng = np.random.RandomState(n_query)
    grid = np.sort(rng.choice(np.arange(1, 4000), size=700, replace=True)) * 0.01      # repeats
    path_t = np.concatenate([[0.0], grid])
    q = rng.uniform(1e-3, path_t.max(), size=n_query)
    on = rng.random_sample(n_query) < 0.3
    q[on] = rng.choice(grid, size=int(on.sum())) + rng.choice([0.0, 5e-11, -5e-11, 2e-10, -2e-10], size=int(on.sum()))
    q = np.minimum(q, path_t.max())
    assert np.array_equal(dev_rows(path_t, q, 'closest'), physionet_eval.get_comparison_times_ind(path_t, q))
    t_vec = np.around(path_t, 2).astype(np.float32)
    assert np.array_equal(dev_rows(t_vec.astype(np.float64), q, 'first_nearest'), first_nearest_on_host(t_vec, q))


def test_rows_on_a_real_schedule():
    b = physionet_eval.make_eval_batch(6, n_grid=240)
    path_t = Schedule(b['times'], b['delta_t'], b['T'], True).path_t
    assert np.any(np.diff(path_t) == 0)                     # jumps repeat a time
    step = b['delta_t']
    grid = np.unique(path_t)[1:]
    q = np.concatenate([grid, grid + 5e-11, grid - 5e-11, grid[:-1] + 0.5 * step, grid[:-1] - 0.5 * step])
    q = q[(q > path_t.min()) & (q < path_t.max() + 1e-10)]
    assert np.array_equal(dev_rows(path_t, q, 'closest'), physionet_eval.get_comparison_times_ind(path_t, q))
    n_dec = climate_eval.n_decimals(step)
    t_vec = np.around(path_t, n_dec).astype(np.float32)
    assert np.array_equal(dev_rows(t_vec.astype(np.float64), q, 'first_nearest'), first_nearest_on_host(t_vec, q))


# ---- scores ---------------------------------------------------------------------------------------
def dense_case(B, T2, dim, seed=0):
    rng = np.random.RandomState(1000 * B + 10 * T2 + dim + seed)
    n_rows = T2 + 3
    rows = rng.randint(0, n_rows, size=T2).astype(np.int32)
    pred = rng.standard_normal((n_rows, B, dim)).astype(np.float32)
    vals = rng.standard_normal((B, T2, dim)).astype(np.float32)
    mask = (rng.random_sample((B, T2, dim)) < 0.3).astype(np.float32)
    mask[rng.random_sample(mask.shape) < 0.05] = 2.0      # a weight in sq_sum, a selection in attr_mse
    mask[0, 0, 0] = 1.0
    if dim > 1:
        mask[0, :, dim - 1] = 0.0                          # an attribute never observed for one patient
    if B > 1:
        mask[B - 1] = 0.0                                  # a patient with nothing observed
    return pred, rows, vals, mask


def dense_expected(pred, rows, vals, mask):
    sel = np.transpose(pred[rows], (1, 0, 2))                                   # the host's path_y
    terms = ((sel - vals) ** 2) * mask
    assert terms.dtype == np.float32
    sq = terms.astype(np.float64).sum()
    n_obs = mask.astype(np.float64).sum()
    m = mask > 0
    e = (sel.astype(np.float64) - vals.astype(np.float64)) ** 2
    cnt = m.sum(axis=1)
    per = np.where(cnt > 0, np.where(m, e, 0.0).sum(axis=1) / np.maximum(cnt, 1), 0.0)
    return sq, n_obs, float(np.mean(np.mean(per, axis=-1)))


def check_scores(tag, out, sq, n_obs, attr, n_terms, chain):
    got = out.cpu().numpy()
    print('{}: sq_sum {!r} / {!r}, n_obs {!r} / {!r}, attr_mse {!r} / {!r}'.format(
        tag, got[0], sq, got[1], n_obs, got[2], attr))
    _record('sq_sum', abs(got[0] - sq), (n_terms - 1) * U * sq)
    _record('attr_mse', abs(got[2] - attr), chain * U * attr)
    assert got[1] == n_obs
    assert got[3] == 0.0
    assert abs(got[0] - sq) <= (n_terms - 1) * U * sq, (got[0], sq)
    assert abs(got[2] - attr) <= chain * U * attr, (got[2], attr)


DENSE = [(B, T2, dim) for B in (1, 6, 50) for T2 in (1, 7, 130) for dim in (1, 5, 41)] + [(2, 3, 300)]


@pytest.mark.parametrize('B,T2,dim', DENSE)
def test_dense_scores(B, T2, dim):
    pred, rows, vals, mask = dense_case(B, T2, dim)
    out = protocol.score(_dev(pred), _dev(rows), vals=_dev(vals), mask=_dev(mask))
    assert out.dtype == torch.float64 and tuple(out.shape) == (4,)
    sq, n_obs, attr = dense_expected(pred, rows, vals, mask)
    assert sq > 0 and attr > 0
    check_scores('dense B {} T2 {} dim {}'.format(B, T2, dim), out, sq, n_obs, attr, B * T2 * dim, T2 + dim + B)
    print('largest error / allowance so far:', WORST)
    # the same call again: the same bits
    again = protocol.score(_dev(pred), _dev(rows), vals=_dev(vals), mask=_dev(mask))
    assert torch.equal(out, again)


def sparse_case(L, dim, B=6, seed=0):
    rng = np.random.RandomState(100 * L + dim + seed)
    n_rows = 40
    stations = np.array([0, 1, 3, 4, 5]) if L > 1 else np.array([3])           # station 2 is absent
    index_val = np.sort(rng.choice(stations, size=L)).astype(np.int32)          # ... others repeat
    rows = rng.randint(0, n_rows, size=L).astype(np.int32)
    pred = rng.standard_normal((n_rows, B, dim)).astype(np.float32)
    X_val = rng.standard_normal((L, dim)).astype(np.float32)
    M_val = (rng.random_sample((L, dim)) < 0.4).astype(np.float32)
    M_val[0, 0] = 1.0
    return pred, rows, X_val, M_val, index_val


@pytest.mark.parametrize('L,dim', [(L, dim) for L in (1, 7, 300) for dim in (1, 5, 41)])
def test_sparse_scores(L, dim):
    pred, rows, X_val, M_val, index_val = sparse_case(L, dim)
    if L >= 7:
        assert 2 not in index_val and len(np.unique(index_val)) < L
    args = lambda: dict(X_val=_dev(X_val), M_val=_dev(M_val), index_val=_dev(index_val))
    out = protocol.score(_dev(pred), _dev(rows), **args())
    p_val = pred[rows, index_val]
    terms = ((X_val - p_val) ** 2) * M_val                                      # climate_eval.evaluate_model
    assert terms.dtype == np.float32
    sq = terms.astype(np.float64).sum()
    assert sq > 0
    check_scores('sparse L {} dim {}'.format(L, dim), out, sq, M_val.astype(np.float64).sum(), 0.0, L * dim, 0)
    assert float(out[2]) == 0.0
    print('largest error / allowance so far:', WORST)
    assert torch.equal(out, protocol.score(_dev(pred), _dev(rows), **args()))


def test_accumulate_adds_each_batch_once():
    a = dense_case(6, 7, 5)
    b = dense_case(3, 130, 5, seed=1)
    call = lambda c, **kw: protocol.score(_dev(c[0]), _dev(c[1]), vals=_dev(c[2]), mask=_dev(c[3]), **kw)
    out_a, out_b = call(a).cpu().numpy(), call(b).cpu().numpy()
    acc = torch.full((4,), 7.5, dtype=torch.float64, device=DEV)
    call(a, out=acc)                                        # overwrites what out held
    assert np.array_equal(acc.cpu().numpy(), out_a)
    call(b, out=acc, accumulate=True)
    want = out_a + out_b                                    # one float64 addition per entry
    want[3] = 0.0
    assert out_b[0] > 0 and out_b[2] > 0
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), want.view(np.uint64))
    # ... and a sparse batch on top of it
    s = sparse_case(7, 5, B=6)
    out_s = protocol.score(_dev(s[0]), _dev(s[1]), X_val=_dev(s[2]), M_val=_dev(s[3]), index_val=_dev(s[4]))
    protocol.score(_dev(s[0]), _dev(s[1]), X_val=_dev(s[2]), M_val=_dev(s[3]), index_val=_dev(s[4]),
                   out=acc, accumulate=True)
    want = want + out_s.cpu().numpy()
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), want.view(np.uint64))
    with pytest.raises(ValueError):
        call(a, accumulate=True)                            # nothing to add to


# ---- stated sizes -----------------------------------------------------------------------------------
BAND = 256
PATTERN = 0xC3


class Banded:
    """``nbytes`` of device memory between two bands of PATTERN; the payload starts filled with
    the pattern as well, so that a word the library did not write is seen too"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((BAND + nbytes + BAND,), PATTERN, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr() + BAND

    def payload(self, dtype):
        return self.buf[BAND:BAND + self.nbytes].clone().view(dtype)

    def intact(self):
        lo, hi = self.buf[:BAND], self.buf[BAND + self.nbytes:]
        return bool((lo == PATTERN).all()) and bool((hi == PATTERN).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('layout,B,nq,dim', [('dense', 6, 130, 41), ('dense', 2, 3, 300), ('dense', 50, 7, 5),
                                             ('sparse', 6, 300, 41), ('sparse', 6, 1, 1)])
def test_buffers_at_their_stated_sizes(layout, B, nq, dim):
    L = _lib.lib()
    if layout == 'dense':
        pred, rows, vals, mask = dense_case(B, nq, dim)
        keep = [_dev(pred), _dev(vals), _dev(mask)]
        job = _lib.NjodeProtocolJob(keep[0].data_ptr(), pred.shape[0], B, dim, nq, None, keep[1].data_ptr(),
                                    keep[2].data_ptr(), None, None, None)
        want = dense_expected(pred, rows, vals, mask)
    else:
        pred, rows, X_val, M_val, index_val = sparse_case(nq, dim, B=B)
        keep = [_dev(pred), _dev(X_val), _dev(M_val), _dev(index_val)]
        job = _lib.NjodeProtocolJob(keep[0].data_ptr(), pred.shape[0], B, dim, nq, None, None, None,
                                    keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr())
        want = ((((X_val - pred[rows, index_val]) ** 2) * M_val).astype(np.float64).sum(),
                M_val.astype(np.float64).sum(), 0.0)
    n_rows = pred.shape[0]
    # rows: written by the library into exactly 4 * nq bytes; any path_t / query will do, the
    # scores are taken at the rows the case drew: query j sits on time rows[j] of a strict path
    path_t = _dev(np.arange(n_rows, dtype=np.float64) + 1.0)
    query = _dev(rows.astype(np.float64) + 1.0)
    g_rows = Banded(4 * nq)
    assert L.njode_protocol_rows(path_t.data_ptr(), n_rows, query.data_ptr(), nq, _lib.ROWS_FIRST_NEAREST,
                                 g_rows.ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert g_rows.intact()
    assert np.array_equal(g_rows.payload(torch.int32).cpu().numpy(), rows)
    job.rows = g_rows.ptr
    need = ctypes.c_size_t(0)
    assert L.njode_protocol_bytes(n_rows, nq, B, dim, ctypes.byref(need)) == 0
    g_out, g_ws = Banded(32), Banded(need.value)
    # one byte short: refused, nothing written
    assert L.njode_protocol_score_f32(ctypes.byref(job), g_out.ptr, 0, g_ws.ptr, need.value - 1,
                                      _stream()) == _lib.E_WORKSPACE
    assert L.njode_last_error()
    torch.cuda.synchronize()
    assert bool((g_out.buf == PATTERN).all()) and bool((g_ws.buf == PATTERN).all())
    assert L.njode_protocol_score_f32(ctypes.byref(job), g_out.ptr, 0, g_ws.ptr, need.value, _stream()) == 0
    torch.cuda.synchronize()
    assert g_out.intact() and g_ws.intact() and g_rows.intact()
    got = g_out.payload(torch.float64).cpu().numpy()
    assert got[1] == want[1] and got[3] == 0.0
    assert got[0] == pytest.approx(want[0], rel=1e-12) and got[2] == pytest.approx(want[2], rel=1e-12)


def test_c_level_refusals():
    L = _lib.lib()
    pred, rows, vals, mask = dense_case(2, 3, 5)
    d_pred, d_rows, d_vals, d_mask = _dev(pred), _dev(rows), _dev(vals), _dev(mask)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    need = ctypes.c_size_t(0)
    assert L.njode_protocol_bytes(6, 3, 2, 5, ctypes.byref(need)) == 0
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=DEV)

    def job(**kw):
        f = dict(pred=d_pred.data_ptr(), n_rows=6, B=2, dim=5, n_query=3, rows=d_rows.data_ptr(),
                 vals=d_vals.data_ptr(), mask=d_mask.data_ptr(), X_val=None, M_val=None, index_val=None)
        f.update(kw)
        return _lib.NjodeProtocolJob(**f)

    def call(j, out_p=out.data_ptr(), ws_p=ws.data_ptr()):
        return L.njode_protocol_score_f32(ctypes.byref(j) if j is not None else None, out_p, 0, ws_p,
                                          need.value, _stream())

    some = d_vals.data_ptr()
    refusals = {'null job': (None,), 'null out': (job(), None), 'null ws': (job(), out.data_ptr(), None),
                'null pred': (job(pred=None),), 'null rows': (job(rows=None),),
                'B = 0': (job(B=0),), 'dim = 0': (job(dim=0),), 'B < 0': (job(B=-1),),
                'n_query < 0': (job(n_query=-1),), 'n_rows < 0': (job(n_rows=-1),),
                'no row': (job(n_rows=0),), 'neither layout': (job(vals=None, mask=None),),
                'both layouts': (job(X_val=some, M_val=some, index_val=d_rows.data_ptr()),),
                'half a dense layout': (job(mask=None),),
                'half a sparse layout': (job(vals=None, mask=None, X_val=some, M_val=some),)}
    for what, args in refusals.items():
        assert call(*args) == _lib.E_BADARG, what
        assert L.njode_last_error(), what
    t = _dev(np.array([0.0, 1.0]))
    r = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    rows_call = lambda p=t.data_ptr(), n=2, q=t.data_ptr(), nq=2, rule=0, o=r.data_ptr(): \
        L.njode_protocol_rows(p, n, q, nq, rule, o, _stream())
    for what, kw in {'null path_t': dict(p=None), 'null query': dict(q=None), 'null rows': dict(o=None),
                     'no row': dict(n=0), 'n_query < 0': dict(nq=-1), 'rule 2': dict(rule=2),
                     'rule -1': dict(rule=-1)}.items():
        assert rows_call(**kw) == _lib.E_BADARG, what
    assert rows_call(nq=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == 0xA5).all()) and bool((r == -5).all())
    assert call(job()) == 0 and rows_call() == 0
    torch.cuda.synchronize()
    assert r.tolist() == [0, 1] and float(out[3]) == 0.0 and float(out[1]) == float(mask.sum())


# ---- end to end ---------------------------------------------------------------------------------
def _physio_batches(g):
    out = []
    for i in range(int(g['n_batches'])):
        p = 'b{}/'.format(i)
        out.append({'times': g[p + 'times'], 'time_ptr': g[p + 'time_ptr'],
                    'X': torch.tensor(g[p + 'X']), 'M': torch.tensor(g[p + 'M']),
                    'obs_idx': torch.tensor(g[p + 'obs_idx'], dtype=torch.long),
                    'batch_size': int(g[p + 'batch_size']), 'times_val': g[p + 'times_val'],
                    'vals_val': g[p + 'vals_val'], 'mask_val': g[p + 'mask_val']})
    return out


def _climate_batches(g):
    out = []
    for i in range(int(g['n_batches'])):
        p = 'b{}/'.format(i)
        out.append({'times': g[p + 'times'], 'time_ptr': g[p + 'time_ptr'],
                    'X': torch.tensor(g[p + 'X']), 'M': torch.tensor(g[p + 'M']),
                    'obs_idx': torch.tensor(g[p + 'obs_idx'], dtype=torch.long),
                    'pat_idx': list(range(int(g[p + 'batch_size']))),
                    'X_val': torch.tensor(g[p + 'X_val']), 'M_val': torch.tensor(g[p + 'M_val']),
                    'times_val': g[p + 'times_val'], 'index_val': g[p + 'index_val']})
    return out


def test_physionet_protocol_end_to_end():
    g = Golden('g8_physionet_eval')
    m = hip_model(g.cfg, g.state_dict())
    batches = _physio_batches(g)
    host = physionet_eval.evaluate_model(m, batches, DEV, g.delta_t, g.T)
    dev = physionet_eval.evaluate_model_device(m, batches, DEV, g.delta_t, g.T)
    print('physionet host {!r}\n          device {!r}'.format(host, dev))
    assert all(isinstance(v, float) for v in dev) and len(dev) == 3
    assert dev[0] == host[0]
    assert dev[1] == pytest.approx(host[1], rel=1e-5)
    assert dev[2] == pytest.approx(host[2], rel=1e-5)
    assert dev[0] == pytest.approx(float(g['loss_val']), rel=LOSS_RTOL)
    assert dev[1] == pytest.approx(float(g['mse_val']), rel=1e-4)
    assert dev[2] == pytest.approx(float(g['mse_val_2']), rel=1e-4)
    # a model that hands its loss to the host gives the same triple
    m2 = hip_model(g.cfg, g.state_dict(), device_outputs=False)
    assert physionet_eval.evaluate_model_device(m2, batches, DEV, g.delta_t, g.T) == dev
    # one batch at the test-layout size
    b = physionet_eval.make_eval_batch(50, n_grid=240)
    host = physionet_eval.evaluate_model(m, [b], DEV, b['delta_t'], b['T'])
    dev = physionet_eval.evaluate_model_device(m, [b], DEV, b['delta_t'], b['T'])
    print('B = 50   host {!r}\n          device {!r}'.format(host, dev))
    assert dev[0] == host[0]
    assert dev[1] == pytest.approx(host[1], rel=1e-5) and dev[2] == pytest.approx(host[2], rel=1e-5)
    # nothing observed in the held-out half: the host arithmetic divides by zero
    with pytest.raises(ZeroDivisionError):
        physionet_eval.evaluate_model_device(m, [dict(batches[0], mask_val=np.zeros_like(batches[0]['mask_val']))],
                                             DEV, g.delta_t, g.T)


def test_climate_protocol_end_to_end():
    g = Golden('g8_climate_eval')
    m = hip_model(g.cfg, g.state_dict())
    batches = _climate_batches(g)
    host = climate_eval.evaluate_model(m, batches, DEV, g.delta_t, g.T)
    dev = climate_eval.evaluate_model_device(m, batches, DEV, g.delta_t, g.T)
    print('climate host {!r}\n        device {!r}'.format(host, dev))
    assert all(isinstance(v, float) for v in dev) and len(dev) == 2
    assert dev[0] == host[0]
    assert dev[1] == pytest.approx(host[1], rel=1e-5)
    assert dev[0] == pytest.approx(float(g['loss_val']), rel=LOSS_RTOL)
    assert dev[1] == pytest.approx(float(g['mse_val']), rel=1e-4)
    with pytest.raises(ZeroDivisionError):
        climate_eval.evaluate_model_device(m, [dict(batches[0], M_val=torch.zeros_like(batches[0]['M_val']))],
                                           DEV, g.delta_t, g.T)
