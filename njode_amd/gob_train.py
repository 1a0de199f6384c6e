"""
``train.train(..., other_model='GRU_ODE_Bayes')``: the reference's baseline run
(``NJODE/train.py:354-392, 514-519, 549-566``) on the GPU model of ``gru_ode_bayes``.

Each step is ``model(...)``, ``loss.backward()``, ``torch.optim.Adam(lr, weight_decay=5e-4).step()``
with ``M = 1``; the evaluation loss is the eval-mode loss of the validation batch; ``evaluate=True``
adds ``NNFOwithBayesianJumps.evaluate`` (the mean half of ``path_p`` against the true conditional
expectation).  Checkpoints and the metric file go through ``run.Run``.  The fused step, the plan
look-ahead, data-parallel shards and ``device_eval`` belong to NJ-ODE and do not apply.

The dropout step counter of the model is set from the epoch at every epoch's start, so a run
resumed from a checkpoint draws the masks the uninterrupted run draws.
"""
import time

import torch

from . import data_utils, gru_ode_bayes, parallel, stock_model
from .run import Run, require_single_process

OTHER_MODELS = ('GRU_ODE_Bayes',)


def check_other_model(other_model, device_eval=False):
    """``ValueError`` for a value the reference's docstring does not list (``train.py:393-395``), for
    more than one rank and for ``device_eval``."""
    if other_model not in OTHER_MODELS:
        raise ValueError("Invalid argument for (option) parameter 'other_model': {!r}; one of {}"
                         .format(other_model, OTHER_MODELS))
    require_single_process("other_model='{}'".format(other_model))
    if device_eval:
        raise ValueError("device_eval does not apply to other_model='{}'".format(other_model))


def train_baseline(dataset_arrays, metadata, options, columns, epochs, batch_size, learning_rate, hidden_size,
                   bias, dropout_rate, test_size, seed, device, evaluate, shuffle_seed, log,
                   max_steps_per_epoch, model_path, model_id, save_every, resume_training, load_best,
                   init_state):
    from .train import _device_batch, compute_optimal_eval_loss, split_indices
    stock_paths, observed_dates, nb_obs = dataset_arrays
    delta_t, T = metadata['dt'], metadata['maturity']
    functions = options.get('func_appl_X')
    funcs = tuple(f for f in (data_utils._get_func(n) for n in (functions or [])) if f)
    mult = len(funcs) + 1
    input_size = metadata['dimension'] * mult

    train_idx, val_idx = split_indices(len(nb_obs), test_size, seed)
    torch.manual_seed(0)
    model = gru_ode_bayes.from_options(input_size, hidden_size, bias, dropout_rate, options).to(device)
    if init_state is not None:
        model.load_state_dict(init_state)
    optimizer = torch.optim.Adam(model.parameters(), lr=learning_rate, weight_decay=0.0005)

    val = data_utils.collate_arrays(stock_paths[val_idx], observed_dates[val_idx], nb_obs[val_idx], delta_t,
                                    funcs)
    stockmodel = stock_model.STOCK_MODELS[metadata['model_name']](**metadata)
    opt_eval_loss = compute_optimal_eval_loss(val, stockmodel, delta_t, T) if mult == 1 else float('nan')
    val_d = _device_batch(val, device)
    val_M = torch.ones_like(val_d['X'])

    run = Run(model_path, model_id, columns, log, best_col=4, save_on_best=True)
    run.resume(model, optimizer, device, resume_training, load_best)

    metrics = []
    while model.epoch <= epochs:
        t0 = time.time()
        model.train()
        order = train_idx[parallel.epoch_permutation(len(train_idx), model.epoch, shuffle_seed)]
        n_steps = (len(order) + batch_size - 1) // batch_size
        if max_steps_per_epoch:
            n_steps = min(n_steps, max_steps_per_epoch)
        model._step_counter = (model.epoch - 1) * n_steps
        loss = None
        for s in range(n_steps):
            mine = order[s * batch_size:(s + 1) * batch_size]
            d = _device_batch(data_utils.collate_arrays(stock_paths[mine], observed_dates[mine], nb_obs[mine],
                                                        delta_t, funcs), device)
            optimizer.zero_grad()
            _, loss, _, _ = model(d['times'], d['time_ptr'], d['X'], torch.ones_like(d['X']), d['obs_idx'],
                                  delta_t, T, d['start_X'], return_path=False, smoother=False)
            loss.backward()
            optimizer.step()
        torch.cuda.synchronize()
        train_time = time.time() - t0

        t0 = time.time()
        with torch.no_grad():
            model.eval()
            _, c_loss, _, _ = model(val_d['times'], val_d['time_ptr'], val_d['X'], val_M, val_d['obs_idx'],
                                    delta_t, T, val_d['start_X'], return_path=False, smoother=False)
            loss_val = float(c_loss)
            row_extra = []
            if evaluate:
                row_extra = [model.evaluate(val_d['times'], val_d['time_ptr'], val_d['X'], val['obs_idx'], delta_t,
                                            T, val_d['start_X'], val['n_obs_ot'], stockmodel)]
        eval_time = time.time() - t0
        train_loss = float('nan') if loss is None else float(loss.detach())
        log("epoch {}, weight={:.5f}, train-loss={:.5f}, optimal-eval-loss={:.5f}, "
            "eval-loss={:.5f}, ".format(model.epoch, model.weight, train_loss, opt_eval_loss, loss_val))
        row = [model.epoch, train_time, eval_time, train_loss, loss_val, opt_eval_loss] + row_extra
        metrics.append(row)
        run.end_of_epoch(model, optimizer, row, save_every)
        run.new_best(model, optimizer, loss_val)
        model.epoch += 1
        model.weight_decay_step()
    return model, metrics
