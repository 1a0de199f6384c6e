"""The record training harness (njode_amd/train_records.py, the reproduction of
physionet_train.py:259-392) on a PhysioNet-shaped model: D = H = 41, width 50, 24 records on a
60-step grid, batches of 8, 2 epochs.  The GPU collate and the host collate feed the same batches,
so whole runs agree bit for bit, and both agree with a loop written out by hand."""
import csv
import os

import numpy as np
import pytest
import torch

from njode_amd import models, parallel, physionet_eval, records, synthetic_physionet, train_records

pytestmark = pytest.mark.gpu

DELTA_T, T = 1.0 / 60, synthetic_physionet.PHYSIONET_T
# 25 generated records without record 1, none of whose rows is observed (its loss term is 0 / 0)
IDS = np.array([0] + list(range(2, 25)))
TRAIN, TEST = IDS[:18], IDS[18:]
KW = dict(batch_size=8, hidden_size=41, dropout_rate=0.1, delta_t=DELTA_T, T=T, log=lambda s: None)


@pytest.fixture(scope='module')
def dataset():
    recs, mn, mx = synthetic_physionet.make_records(25, 41, n_quant=60, n_obs_range=(4, 12), seed=7)
    return records.RecordDataset.from_records(recs, mn, mx, device='cuda')


@pytest.fixture(scope='module')
def runs(dataset):
    """The same two epochs through the GPU collate and through the host collate."""
    dev = train_records.train_records(dataset, TRAIN, TEST, epochs=2, device_collate=True, **KW)
    host = train_records.train_records(dataset, TRAIN, TEST, epochs=2, device_collate=False, **KW)
    return dev, host


def _values(metrics):
    return [[r[0]] + r[3:] for r in metrics]          # without the two wall-clock columns


def test_device_and_host_collate_train_identically(runs):
    (m1, met1), (m2, met2) = runs
    assert len(met1) == 2 and all(len(r) == len(train_records.METR_COLUMNS) for r in met1)
    assert _values(met1) == _values(met2)
    assert torch.equal(m1.flat_parameters(), m2.flat_parameters())
    assert m1.epoch == 3 and m1.masked
    assert all(np.isfinite(r[3:]).all() for r in met1)
    assert train_records.METR_COLUMNS == ['epoch', 'train_time', 'eval_time', 'train_loss',
                                          'eval_loss', 'eval_metric', 'eval_metric_2']


def test_loop_written_out_by_hand(dataset, runs):
    """collate_host + loss_and_grad + FusedAdam.step in the harness's order; the evaluation on
    host-collated test batches gives the triple the harness got on device-collated ones."""
    (m1, met1), _ = runs
    torch.manual_seed(0)
    model = models.NJODE(41, 41, 41, train_records.NN, train_records.NN, train_records.NN, False,
                         bias=True, dropout_rate=0.1, solver='euler', weight=0.5, weight_decay=1.,
                         options={'masked': True, 'device_outputs': True}).to('cuda')
    opt = models.FusedAdam(model, lr=1e-3, weight_decay=0.0005)
    test_batches = [dataset.collate_host(TEST[i:i + 8], 'test') for i in range(0, len(TEST), 8)]
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
        triple = physionet_eval.evaluate_model_device(model, test_batches, 'cuda', DELTA_T, T)
        rows.append([epoch, float(loss)] + list(triple))
        model.epoch += 1
        model.weight_decay_step()
    assert rows == _values(met1)
    assert torch.equal(model.flat_parameters(), m1.flat_parameters())


def test_evaluation_takes_resident_held_out_arrays(dataset, runs):
    (m1, _), _ = runs
    lists = [TEST[:4], TEST[4:]]
    on_dev = [dataset.fill_batch(p) for p in dataset.prepare_batches(lists, 'test')]
    on_host = [dataset.collate_host(ix, 'test') for ix in lists]
    assert on_dev[0]['vals_val'].is_cuda and isinstance(on_host[0]['vals_val'], np.ndarray)
    a = physionet_eval.evaluate_model_device(m1, on_dev, 'cuda', DELTA_T, T)
    b = physionet_eval.evaluate_model_device(m1, on_host, 'cuda', DELTA_T, T)
    assert a == b and np.isfinite(a).all()
    # the shape check is the same for resident arrays
    wrong = dict(on_dev[0], vals_val=on_dev[0]['vals_val'][:, :-1].contiguous())
    with pytest.raises(ValueError, match='vals_val must be'):
        physionet_eval.evaluate_model_device(m1, [wrong], 'cuda', DELTA_T, T)


def test_unfused_route_tracks_the_fused_one(dataset, runs):
    (m1, met1), _ = runs
    m3, met3 = train_records.train_records(dataset, TRAIN, TEST, epochs=2, fused=False, **KW)
    np.testing.assert_allclose(m3.flat_parameters().cpu().numpy(), m1.flat_parameters().cpu().numpy(),
                               atol=5e-5, rtol=1e-3)
    assert met3[1][4] == pytest.approx(met1[1][4], rel=1e-3)


def test_checkpoints_metric_file_and_resume(dataset, tmp_path):
    kw = dict(KW, dropout_rate=0.0, model_path=str(tmp_path), model_id=4)
    m1, met1 = train_records.train_records(dataset, TRAIN, TEST, epochs=1, **kw)
    d = os.path.join(str(tmp_path), 'id-4')
    for name in ('last_checkpoint', 'best_checkpoint'):
        ck = torch.load(os.path.join(d, name, 'checkpt.tar'), weights_only=False)
        assert set(ck) == {'epoch', 'weight', 'model_state_dict', 'optimizer_state_dict'}
        assert ck['epoch'] == 1
    rows = list(csv.reader(open(os.path.join(d, 'metric_id-4.csv'))))
    assert rows[0] == [''] + train_records.METR_COLUMNS and len(rows) == 2 and rows[1][0] == '0'
    assert float(rows[1][1]) == 1 and float(rows[1][6]) == met1[0][5]
    # two epochs in one go == one epoch, then a resumed run for the second
    m2, met2 = train_records.train_records(dataset, TRAIN, TEST, epochs=2, resume_training=True, **kw)
    m3, met3 = train_records.train_records(dataset, TRAIN, TEST, epochs=2,
                                           **dict(KW, dropout_rate=0.0))
    assert len(met2) == 1 and met2[0][0] == 2 and m2.epoch == 3
    assert torch.equal(m2.flat_parameters(), m3.flat_parameters())
    assert _values(met2) == _values(met3)[1:]
    rows = list(csv.reader(open(os.path.join(d, 'metric_id-4.csv'))))
    assert [r[0] for r in rows[1:]] == ['0', '1'] and [float(r[1]) for r in rows[1:]] == [1, 2]
    best = torch.load(os.path.join(d, 'best_checkpoint', 'checkpt.tar'), weights_only=False)
    assert best['epoch'] == 1 + int(np.argmin([met1[0][5], met2[0][5]]))
    # save_every = 2: the metric file and the last checkpoint wait for the second epoch
    kw2 = dict(kw, model_id=5, save_every=2)
    train_records.train_records(dataset, TRAIN, TEST, epochs=1, **kw2)
    d5 = os.path.join(str(tmp_path), 'id-5')
    assert not os.path.exists(os.path.join(d5, 'last_checkpoint', 'checkpt.tar'))
    assert os.path.exists(os.path.join(d5, 'best_checkpoint', 'checkpt.tar'))
    assert not os.path.exists(os.path.join(d5, 'metric_id-5.csv'))


def test_refusals(dataset, monkeypatch):
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(ValueError, match='single process'):
        train_records.train_records(dataset, TRAIN, TEST, epochs=1, **KW)
    monkeypatch.undo()
    with pytest.raises(ValueError):
        train_records.train_records(dataset, [], TEST, epochs=1, **KW)
    host_only = records.RecordDataset(dataset.grid, dataset.row_ptr, dataset.row_g, dataset.vals,
                                      dataset.mask, dataset.att_min, dataset.att_max, True, None)
    with pytest.raises(ValueError, match='resident'):
        train_records.train_records(host_only, TRAIN, TEST, epochs=1, **KW)
