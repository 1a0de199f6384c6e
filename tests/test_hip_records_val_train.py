"""The climate training harness (njode_amd/train_records.py: ``train_climate_records``, the
reproduction of climate_train.py:356-488) on the climate shape: D = 5, H = 10, width 50, 40
synthetic stations, batches of 8, 2 epochs, a coarse step (delta_t = 1: about 200 Euler steps
plus the observation times).  The GPU collate and the host collate feed the same batches, so
whole runs agree bit for bit, and both agree with a loop written out by hand."""
import csv
import os

import numpy as np
import pytest
import torch

from njode_amd import climate_eval, models, parallel, records, synthetic_physionet, train_records

pytestmark = pytest.mark.gpu

DELTA_T, T, T_VAL = 1.0, 200, 150
TRAIN, VAL, TEST = np.arange(0, 24), np.arange(24, 32), np.arange(32, 40)
KW = dict(batch_size=8, hidden_size=10, dropout_rate=0.1, delta_t=DELTA_T, log=lambda s: None)
COLUMNS = ['epoch', 'train_time', 'eval_time', 'train_loss', 'eval_loss', 'eval_metric',
           'test_loss', 'test_metric']


def _records():
    recs = synthetic_physionet.make_climate_records(40, 5, n_obs_range=(6, 14), seed=23)
    # stations the validation and the test set must drop: one ends before T_val, one starts after
    recs[25] = tuple(a[recs[25][0] <= T_VAL] for a in recs[25])
    recs[34] = tuple(a[recs[34][0] > T_VAL] for a in recs[34])
    return recs


@pytest.fixture(scope='module')
def dataset():
    return records.RecordDataset.from_records(_records(), time_div=None, drop_unobserved=False,
                                              device='cuda')


@pytest.fixture(scope='module')
def runs(dataset):
    """The same two epochs through the GPU collate and through the host collate."""
    dev = train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=2,
                                              device_collate=True, **KW)
    host = train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=2,
                                               device_collate=False, **KW)
    return dev, host


def _values(metrics):
    return [[r[0]] + r[3:] for r in metrics]          # without the two wall-clock columns


def test_device_and_host_collate_train_identically(dataset, runs):
    (m1, met1), (m2, met2) = runs
    assert train_records.CLIMATE_METR_COLUMNS == COLUMNS
    assert len(met1) == 2 and all(len(r) == 8 for r in met1)
    assert _values(met1) == _values(met2)
    assert torch.equal(m1.flat_parameters(), m2.flat_parameters())
    assert m1.epoch == 3 and m1.masked
    assert all(np.isfinite(r[3:]).all() for r in met1)
    kept = dataset.eligible(VAL, T_VAL)
    assert 0 < len(kept) < len(VAL) and 25 not in kept
    assert 34 not in dataset.eligible(TEST, T_VAL)


def test_loop_written_out_by_hand(dataset, runs):
    """collate_host + loss_and_grad + FusedAdam.step in the harness's order, then the protocol on
    the device-collated validation and test batch."""
    (m1, met1), _ = runs
    torch.manual_seed(0)
    model = models.NJODE(5, 10, 5, train_records.NN, train_records.NN, train_records.NN, False,
                         bias=True, dropout_rate=0.1, solver='euler', weight=0.5, weight_decay=1.,
                         options={'masked': True, 'device_outputs': True}).to('cuda')
    opt = models.FusedAdam(model, lr=1e-3, weight_decay=0.0005)
    val_b = dataset.collate_val(dataset.eligible(VAL, T_VAL), T_VAL, 3)
    test_b = dataset.collate_val(dataset.eligible(TEST, T_VAL), T_VAL, 3)
    rows = []
    for epoch in (1, 2):
        assert model.epoch == epoch
        model.train()
        order = TRAIN[parallel.epoch_permutation(len(TRAIN), epoch, 0)]
        for s in range(0, len(order), 8):
            b = dataset.collate_host(order[s:s + 8], 'train')
            opt.zero_grad()
            _, loss = model.loss_and_grad(
                b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), DELTA_T, T,
                b['start_X'].cuda(), b['n_obs_ot'].cuda().int(), M=b['M'].cuda())
            opt.step()
        pair_val = climate_eval.evaluate_model_device(model, [val_b], 'cuda', DELTA_T, T)
        pair_test = climate_eval.evaluate_model_device(model, [test_b], 'cuda', DELTA_T, T)
        rows.append([epoch, float(loss)] + list(pair_val) + list(pair_test))
        model.epoch += 1
        model.weight_decay_step()
    assert rows == _values(met1)
    assert torch.equal(model.flat_parameters(), m1.flat_parameters())


def test_resident_batch_against_the_host_protocol(dataset, runs):
    """``evaluate_model_device`` on the arrays in HBM against ``evaluate_model`` (numpy
    ``extract_from_path`` and fp32 sums on the host) on the host-collated batch: the loss is the
    same model call, the MSE differs by its summation (float64 on the device) -- 1e-5 relative,
    the bound between the two protocol routes."""
    (m1, _), _ = runs
    idx = dataset.eligible(VAL, T_VAL)
    on_dev, on_host = dataset.collate_val(idx, T_VAL, 3), dataset.collate_val_host(idx, T_VAL, 3)
    assert on_dev['X_val'].is_cuda and on_dev['times_val'].is_cuda and on_dev['index_val'].is_cuda
    a = climate_eval.evaluate_model_device(m1, [on_dev], 'cuda', DELTA_T, T)
    b = climate_eval.evaluate_model(m1, [on_host], 'cuda', DELTA_T, T)
    print('device route', a, 'host route', b)
    assert a[0] == b[0]
    assert a[1] == pytest.approx(b[1], rel=1e-5)
    # the same call on the host-collated arrays takes the upload path: the same bits
    assert climate_eval.evaluate_model_device(m1, [on_host], 'cuda', DELTA_T, T) == a
    # the shape check holds for resident arrays too
    wrong = dict(on_dev, X_val=on_dev['X_val'][:, :-1].contiguous())
    with pytest.raises(ValueError, match='X_val must be'):
        climate_eval.evaluate_model_device(m1, [wrong], 'cuda', DELTA_T, T)


def test_checkpoints_metric_file_and_resume(dataset, tmp_path):
    kw = dict(KW, dropout_rate=0.0, model_path=str(tmp_path), model_id=4)
    m1, met1 = train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=1, **kw)
    d = os.path.join(str(tmp_path), 'id-4')
    for name in ('last_checkpoint', 'best_checkpoint'):
        ck = torch.load(os.path.join(d, name, 'checkpt.tar'), weights_only=False)
        assert set(ck) == {'epoch', 'weight', 'model_state_dict', 'optimizer_state_dict'}
        assert ck['epoch'] == 1
    rows = list(csv.reader(open(os.path.join(d, 'metric_id-4.csv'))))
    assert rows[0] == [''] + COLUMNS and len(rows) == 2 and rows[1][0] == '0'
    assert float(rows[1][1]) == 1 and float(rows[1][6]) == met1[0][5] and float(rows[1][8]) == met1[0][7]
    # two epochs in one go == one epoch, then a resumed run for the second
    m2, met2 = train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=2,
                                                   resume_training=True, **kw)
    m3, met3 = train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=2,
                                                   **dict(KW, dropout_rate=0.0))
    assert len(met2) == 1 and met2[0][0] == 2 and m2.epoch == 3
    assert torch.equal(m2.flat_parameters(), m3.flat_parameters())
    assert _values(met2) == _values(met3)[1:]
    rows = list(csv.reader(open(os.path.join(d, 'metric_id-4.csv'))))
    assert [r[0] for r in rows[1:]] == ['0', '1'] and [float(r[1]) for r in rows[1:]] == [1, 2]
    best = torch.load(os.path.join(d, 'best_checkpoint', 'checkpt.tar'), weights_only=False)
    assert best['epoch'] == 1 + int(np.argmin([met1[0][5], met2[0][5]]))


def test_refusals(dataset, monkeypatch):
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(ValueError, match='single process'):
        train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=1, **KW)
    monkeypatch.undo()
    # an empty eligible set: the only validation record ends before T_val / nothing lies after it
    with pytest.raises(ValueError, match='T_val'):
        train_records.train_climate_records(dataset, TRAIN, [25], TEST, epochs=1, **KW)
    with pytest.raises(ValueError, match='T_val'):
        train_records.train_climate_records(dataset, TRAIN, VAL, [34], epochs=1, **KW)
    with pytest.raises(ValueError, match='T_val'):
        train_records.train_climate_records(dataset, TRAIN, VAL, TEST, epochs=1, T_val=1000, **KW)
    with pytest.raises(ValueError):
        train_records.train_climate_records(dataset, [], VAL, TEST, epochs=1, **KW)
    host_only = records.RecordDataset(dataset.grid, dataset.row_ptr, dataset.row_g, dataset.vals,
                                      dataset.mask, None, None, False, None)
    with pytest.raises(ValueError, match='resident'):
        train_records.train_climate_records(host_only, TRAIN, VAL, TEST, epochs=1, **KW)
