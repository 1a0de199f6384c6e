"""
Training / evaluation loop of the masked NJ-ODE model on a dataset of irregular records.

Reproduces the compute semantics of the reference harness ``NJODE/physionet_train.py:259-392``
-- nothing of its experiment management (model-id registry, parser, Telegram) -- on a
``records.RecordDataset``:

* model with ``options['masked'] = True``, ``Adam(lr, weight_decay=0.0005)`` (``:152, 259-269``);
* per optimizer step (``:328-353``): the train-layout collate of the batch, ``n_obs_ot`` counted
  from ``obs_idx``, ``start_X = 0``, ``model(..., M=M)`` in train mode, backward, step;
* per epoch (``:356-392``): ``evaluate_model`` on the test-layout batches of the test records
  (observe the first half of each batch's time axis, score the second half), ``train_loss`` =
  the last batch's loss, one metric row of ``METR_COLUMNS``, ``best_checkpoint`` on a lower
  ``eval_metric``, ``last_checkpoint`` + metric file every ``save_every`` epochs,
  ``model.epoch += 1``, ``model.weight_decay_step()``;
* ``resume_training`` / ``load_best`` (``:274-292``) continue from those checkpoints.

Batches follow ``parallel.epoch_permutation`` like ``train.train``.  The fused step
(``NJODE.loss_and_grad`` + ``FusedAdam``) is the default; ``fused=False`` drives the model like
the reference (``loss.backward()`` + ``torch.optim.Adam``).  Single process only.

``train_climate_records`` is the same loop for the third entry point of the reference,
``NJODE/climate_train.py:356-488``: a validation and a test set, each one batch in the climate
validation layout, scored after every epoch (``climate_eval.evaluate_model_device``).
"""
import time

import numpy as np
import torch

from . import climate_eval, parallel, physionet_eval, synthetic_physionet
from .run import Run, new_model_and_optimizer, plan_ahead_on, require_single_process, wants_prefetch

METR_COLUMNS = ['epoch', 'train_time', 'eval_time', 'train_loss', 'eval_loss', 'eval_metric',
                'eval_metric_2']
NN = ((50, 'tanh'), (50, 'tanh'))


def _upload(b, device):
    """A ``collate_host`` batch with the tensors of the step on the device (held-out arrays stay
    numpy: ``evaluate_model_device`` uploads them per call)."""
    d = dict(b)
    for k in ('X', 'M', 'start_X'):
        d[k] = b[k].to(device)
    d['obs_idx'] = b['obs_idx'].to(device, torch.int32)
    d['n_obs_ot'] = b['n_obs_ot'].to(device, torch.int32)
    return d


def _epoch_steps(model, optimizer, dataset, lists, prepared, dev, delta_t, T, fused, plan_ahead):
    """The optimizer steps of one epoch on the train-layout batches of the records ``lists``
    (``prepared``: their ``prepare_batches`` descriptors, or None for the host collate), the next
    batch collated -- and its plan prefetched -- beside the current step.  Returns the last
    batch's loss."""
    def prepare(s):
        if prepared is not None:
            return dataset.fill_batch(prepared[s])
        return _upload(dataset.collate_host(lists[s], 'train'), dev)

    loss = None
    nxt = prepare(0)
    for s in range(len(lists)):
        d = nxt
        nxt = prepare(s + 1) if s + 1 < len(lists) else None
        if plan_ahead and fused and nxt is not None and wants_prefetch(
                model, nxt['batch_size'], int(nxt['time_ptr'][-1])):
            model.prefetch_plan(nxt['times'], nxt['time_ptr'], nxt['X'], nxt['obs_idx'], delta_t,
                                T, nxt['start_X'], nxt['n_obs_ot'], M=nxt['M'], need_hT=True)
        args = (d['times'], d['time_ptr'], d['X'], d['obs_idx'], delta_t, T, d['start_X'],
                d['n_obs_ot'])
        optimizer.zero_grad()
        if fused:
            _, loss = model.loss_and_grad(*args, M=d['M'])
        else:
            _, loss = model(*args, return_path=False, get_loss=True, M=d['M'])
            loss.backward()
        optimizer.step()
    return loss


def train_records(dataset, train_idx, test_idx, epochs=1, batch_size=50, learning_rate=1e-3,
                  hidden_size=41, bias=True, dropout_rate=0.1, ode_nn=NN, readout_nn=NN, enc_nn=NN,
                  use_rnn=False, solver='euler', weight=0.5, weight_decay=1.,
                  delta_t=synthetic_physionet.PHYSIONET_DELTA_T, T=synthetic_physionet.PHYSIONET_T,
                  device='cuda', fused=True, device_collate=True, shuffle_seed=0, log=print,
                  model_path=None, model_id=1, save_every=1, resume_training=False,
                  load_best=False, plan_ahead=True, init_state=None, **options):
    """Train on the records ``train_idx`` of ``dataset`` (a ``records.RecordDataset``), evaluate on
    ``test_idx`` after every epoch.  Returns ``(model, metrics)`` with one row of ``METR_COLUMNS``
    per epoch.

    ``device_collate=True`` builds every batch with the GPU collate of the resident store -- phase
    1 for a whole epoch at once (one upload, one copy back, one wait), phase 2 one batch ahead,
    and the next batch's execution plan prefetched beside the current step under the conditions
    ``train.train`` applies; the test batches, held-out arrays included, are built once and stay in
    HBM.  ``device_collate=False`` collates on the host (``collate_host``) and uploads: the same
    batches, bit for bit.  ``ValueError`` under a process group of more than one rank."""
    require_single_process('train_records')
    train_idx = np.asarray(train_idx, dtype=np.int64).reshape(-1)
    test_idx = np.asarray(test_idx, dtype=np.int64).reshape(-1)
    if len(train_idx) == 0 or len(test_idx) == 0 or batch_size <= 0:
        raise ValueError('train_idx, test_idx and batch_size must not be empty')
    if device_collate and dataset.device is None:
        raise ValueError('device_collate needs a RecordDataset resident on the GPU')
    dev = torch.device(device)
    model, optimizer = new_model_and_optimizer(
        (dataset.dim, hidden_size, dataset.dim), (ode_nn, readout_nn, enc_nn), use_rnn, dev,
        dict(options, masked=True), fused, learning_rate, init_state, bias=bias,
        dropout_rate=dropout_rate, solver=solver, weight=weight, weight_decay=weight_decay)

    # the test batches never change: collated once, in the records' order
    test_lists = [test_idx[i:i + batch_size] for i in range(0, len(test_idx), batch_size)]
    if device_collate:
        test_batches = [dataset.fill_batch(p) for p in dataset.prepare_batches(test_lists, 'test')]
    else:
        test_batches = [_upload(dataset.collate_host(ix, 'test'), dev) for ix in test_lists]

    run = Run(model_path, model_id, METR_COLUMNS, log, best_col=5, save_on_best=False)
    run.resume(model, optimizer, dev, resume_training, load_best)

    def plan_epoch(epoch):
        order = train_idx[parallel.epoch_permutation(len(train_idx), epoch, shuffle_seed)]
        lists = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
        return lists, dataset.prepare_batches(lists, 'train') if device_collate else None

    plan_ahead = plan_ahead_on(plan_ahead)
    metrics, epoch_plan = [], {}
    while model.epoch <= epochs:
        t0 = time.time()
        model.train()
        lists, prepared = epoch_plan.pop(model.epoch, None) or plan_epoch(model.epoch)
        loss = _epoch_steps(model, optimizer, dataset, lists, prepared, dev, delta_t, T, fused,
                            plan_ahead)
        # the next epoch's order and collate counts, queued behind this epoch's steps: their one
        # host wait is the end-of-epoch wait the loop needs anyway
        if device_collate and model.epoch + 1 <= epochs:
            epoch_plan[model.epoch + 1] = plan_epoch(model.epoch + 1)
        torch.cuda.synchronize(dev)
        train_time = time.time() - t0

        t0 = time.time()
        loss_val, mse_val, mse_val_2 = physionet_eval.evaluate_model_device(
            model, test_batches, dev, delta_t, T)
        eval_time = time.time() - t0
        train_loss = float(loss.detach())
        log("epoch {}, weight={:.5f}, train-loss={:.5f}, eval-loss={:.5f}, eval-metric={:.5f}, "
            "eval-metric_2={:.5f}".format(model.epoch, model.weight, train_loss, loss_val, mse_val,
                                          mse_val_2))
        row = [model.epoch, train_time, eval_time, train_loss, loss_val, mse_val, mse_val_2]
        metrics.append(row)
        run.new_best(model, optimizer, mse_val)
        run.end_of_epoch(model, optimizer, row, save_every)
        model.epoch += 1
        model.weight_decay_step()
    return model, metrics


CLIMATE_METR_COLUMNS = ['epoch', 'train_time', 'eval_time', 'train_loss', 'eval_loss',
                        'eval_metric', 'test_loss', 'test_metric']


def train_climate_records(dataset, train_idx, val_idx, test_idx, epochs=1, batch_size=100,
                          learning_rate=1e-3, hidden_size=10, bias=True, dropout_rate=0.1,
                          ode_nn=NN, readout_nn=NN, enc_nn=NN, use_rnn=False, solver='euler',
                          weight=0.5, weight_decay=1., T=climate_eval.CLIMATE_T,
                          T_val=climate_eval.CLIMATE_T_VAL, max_val_samples=3, device='cuda',
                          fused=True, device_collate=True, shuffle_seed=0, log=print,
                          model_path=None, model_id=1, save_every=1, resume_training=False,
                          load_best=False, plan_ahead=True, init_state=None, **options):
    """The compute semantics of ``NJODE/climate_train.py:356-488`` on a ``records.RecordDataset``
    of climate records (every row kept, values raw): train on whole records ``train_idx`` in the
    train layout; after every epoch ``evaluate_model`` on the validation set and on the test set,
    each ONE batch of its eligible records (``dataset.eligible``: a row up to ``T_val`` and a row
    after it) in the validation layout (observe up to ``T_val``, score the next
    ``max_val_samples`` rows of every record), collated once, in the records' order.  Returns
    ``(model, metrics)`` with one row of ``CLIMATE_METR_COLUMNS`` per epoch; ``best_checkpoint``
    follows the validation MSE.  ``delta_t`` is the reference's option (default 0.1).

    ``device_collate``, ``fused``, ``resume_training`` / ``load_best`` as in ``train_records``.
    ``ValueError`` for an empty eligible validation or test set and under a process group of more
    than one rank."""
    require_single_process('train_climate_records')
    train_idx = np.asarray(train_idx, dtype=np.int64).reshape(-1)
    if len(train_idx) == 0 or batch_size <= 0:
        raise ValueError('train_idx and batch_size must not be empty')
    if device_collate and dataset.device is None:
        raise ValueError('device_collate needs a RecordDataset resident on the GPU')
    val_idx, test_idx = dataset.eligible(val_idx, T_val), dataset.eligible(test_idx, T_val)
    if len(val_idx) == 0 or len(test_idx) == 0:
        raise ValueError('no record of the validation or of the test set has a row up to T_val = '
                         '{} and a row after it'.format(T_val))
    dev = torch.device(device)
    model_opts = dict(options, masked=True)
    delta_t = model_opts.pop('delta_t', climate_eval.CLIMATE_DELTA_T)
    model, optimizer = new_model_and_optimizer(
        (dataset.dim, hidden_size, dataset.dim), (ode_nn, readout_nn, enc_nn), use_rnn, dev,
        model_opts, fused, learning_rate, init_state, bias=bias, dropout_rate=dropout_rate,
        solver=solver, weight=weight, weight_decay=weight_decay)

    # the validation and the test set never change: one batch each, collated once
    if device_collate:
        val_batch, test_batch = (dataset.fill_batch(p) for p in dataset.prepare_val_batches(
            [val_idx, test_idx], T_val, max_val_samples))
    else:
        val_batch, test_batch = (_upload(dataset.collate_val_host(ix, T_val, max_val_samples), dev)
                                 for ix in (val_idx, test_idx))

    run = Run(model_path, model_id, CLIMATE_METR_COLUMNS, log, best_col=5, save_on_best=False)
    run.resume(model, optimizer, dev, resume_training, load_best)

    def plan_epoch(epoch):
        order = train_idx[parallel.epoch_permutation(len(train_idx), epoch, shuffle_seed)]
        lists = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
        return lists, dataset.prepare_batches(lists, 'train') if device_collate else None

    plan_ahead = plan_ahead_on(plan_ahead)
    metrics, epoch_plan = [], {}
    while model.epoch <= epochs:
        t0 = time.time()
        model.train()
        lists, prepared = epoch_plan.pop(model.epoch, None) or plan_epoch(model.epoch)
        loss = _epoch_steps(model, optimizer, dataset, lists, prepared, dev, delta_t, T, fused,
                            plan_ahead)
        if device_collate and model.epoch + 1 <= epochs:
            epoch_plan[model.epoch + 1] = plan_epoch(model.epoch + 1)
        torch.cuda.synchronize(dev)
        train_time = time.time() - t0

        t0 = time.time()
        loss_val, mse_val = climate_eval.evaluate_model_device(model, [val_batch], dev, delta_t, T)
        eval_time = time.time() - t0
        train_loss = float(loss.detach())
        log("epoch {}, weight={:.5f}, train-loss={:.5f}, eval-loss={:.5f}, eval-metric={:.5f}".format(
            model.epoch, model.weight, train_loss, loss_val, mse_val))
        run.new_best(model, optimizer, mse_val)
        loss_test, mse_test = climate_eval.evaluate_model_device(model, [test_batch], dev, delta_t, T)
        log("test-loss={:.5f}, test-metric={:.5f}".format(loss_test, mse_test))
        row = [model.epoch, train_time, eval_time, train_loss, loss_val, mse_val, loss_test,
               mse_test]
        metrics.append(row)
        run.end_of_epoch(model, optimizer, row, save_every)
        model.epoch += 1
        model.weight_decay_step()
    return model, metrics
