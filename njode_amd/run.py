"""
What ``train.train``, ``train_records.train_records`` and ``train_records.train_climate_records``
share: the model and optimizer of a run, the switches of the plan look-ahead, and the files of one
model id -- checkpoints, metric file, resume.
"""
import csv
import os

import numpy as np
import torch

from . import models, parallel


def require_single_process(name):
    """``ValueError`` under a process group of more than one rank."""
    if torch.distributed.is_available() and torch.distributed.is_initialized() \
            and torch.distributed.get_world_size() > 1:
        raise ValueError('{} is single process: multi-GPU record training is not offered'.format(name))


def new_model_and_optimizer(sizes, nets, use_rnn, device, options, fused, learning_rate, init_state=None,
                            world=1, **model_kw):
    """The seed-0 model (``sizes`` = input, hidden, output; ``nets`` = ode, readout, encoder) with
    device outputs on ``device``, optionally started from ``init_state``, and its optimizer:
    ``FusedAdam`` or ``torch.optim.Adam``, ``weight_decay=0.0005`` as the reference harness sets."""
    options = dict(options, device_outputs=True)
    torch.manual_seed(0)
    model = models.NJODE(sizes[0], sizes[1], sizes[2], nets[0], nets[1], nets[2], use_rnn,
                         options=options, **model_kw).to(device)
    if init_state is not None:     # start from given weights (like-for-like runs against the reference)
        model.load_state_dict(init_state)
    if world > 1:
        parallel.broadcast_parameters_(model.flat_parameters())
    if fused:
        optimizer = models.FusedAdam(model, lr=learning_rate, weight_decay=0.0005, distributed=world > 1)
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=learning_rate, weight_decay=0.0005)
    return model, optimizer


def plan_ahead_on(plan_ahead):
    """(NJODE_PLAN_AHEAD=0: A/B switch for the look-ahead)"""
    return bool(plan_ahead) and os.environ.get('NJODE_PLAN_AHEAD', '1') != '0'


def wants_prefetch(model, n_next, n_obs_next, plan_ahead_min=0):
    """Whether the plan of the next batch (``n_next`` paths, ``n_obs_next`` observation rows) is
    prefetched beside the current fused step.  Where it pays (profiles/r03_harness_epochs.jsonl,
    epoch paths/s with / without): B = 100: 316 k / 297 k, B = 200: 572 k / 524 k -- the step is a
    chain of ~5 us launches and the plan's six are off it; B = 1 000: 1.83 M / 2.04 M -- the plan
    kernels queued ahead delay the step's own; B >= 4 096: the plan (~0.1 ms) hides beside the ODE
    kernels (bench.py: 1.19 -> 1.14 ms at 20 000 paths).  Up to ~260 000 rows a deferred plan rides
    inside the step's ODE-forward launch and pays at every size (``NJODE.plan_defer_ok``; never
    for a masked model)."""
    return n_next >= max(plan_ahead_min, 1) and (n_next <= 512 or n_next >= 4096
                                                 or model.plan_defer_ok(n_obs_next))


class Run:
    """Checkpoints, metric file and resume of one model id under ``model_path`` (None: nothing is
    written).  ``best_col``: the column of a metric row that ``best_checkpoint`` follows;
    ``save_on_best``: an improvement also writes ``last_checkpoint`` and the metric file, which
    otherwise happens every ``save_every`` epochs only; ``writes=False`` (a rank other than 0)
    resumes but writes nothing."""

    def __init__(self, model_path, model_id, columns, log, best_col, save_on_best, writes=True):
        self.columns, self.log, self.best_col, self.save_on_best = columns, log, best_col, save_on_best
        self.best = np.inf
        self.path_last = self.path_best = self.metric_file = None
        self.saved_rows, self.pending = [], []
        self.writes = writes and model_path is not None
        if model_path is not None:
            model_dir = os.path.join(model_path, 'id-{}'.format(model_id))
            self.path_last = os.path.join(model_dir, 'last_checkpoint')
            self.path_best = os.path.join(model_dir, 'best_checkpoint')
            self.metric_file = os.path.join(model_dir, 'metric_id-{}.csv'.format(model_id))
            os.makedirs(model_dir, exist_ok=True)

    def resume(self, model, optimizer, dev, resume_training, load_best):
        if self.metric_file is None or not resume_training:
            return
        path = self.path_best if load_best else self.path_last
        if not os.path.exists(os.path.join(path, 'checkpt.tar')):
            return
        models.get_ckpt_model(path, model, optimizer, dev)
        if os.path.exists(self.metric_file):
            with open(self.metric_file) as f:
                self.saved_rows = [[float(x) for x in r[1:]] for r in list(csv.reader(f))[1:]]
            if self.saved_rows:
                self.best = min(r[self.best_col] for r in self.saved_rows)
        model.epoch += 1
        model.weight_decay_step()

    def write_metrics(self):
        # pandas' DataFrame.to_csv layout: unnamed index column first
        with open(self.metric_file, 'w', newline='') as f:
            wr = csv.writer(f)
            wr.writerow([''] + self.columns)
            for i, r in enumerate(self.saved_rows):
                wr.writerow([i] + r)

    def new_best(self, model, optimizer, value):
        """``best_checkpoint`` when the followed column improves."""
        if not self.writes or not value < self.best:
            return
        what = self.columns[self.best_col][len('eval_'):]       # 'loss' / 'metric'
        self.log('save new best model: last-best-{0}: {1:.5f}, new-best-{0}: {2:.5f}, '
                 'epoch: {3}'.format(what, self.best, value, model.epoch))
        models.save_checkpoint(model, optimizer, self.path_best, model.epoch)
        self.best = value

    def end_of_epoch(self, model, optimizer, row, save_every):
        """The epoch's metric row; ``last_checkpoint`` + metric file every ``save_every`` epochs --
        with ``save_on_best`` also for a row that improves (call it before ``new_best``)."""
        self.pending.append(row)
        if self.writes and (model.epoch % save_every == 0
                            or (self.save_on_best and row[self.best_col] < self.best)):
            self.saved_rows.extend(self.pending)
            self.pending = []
            self.write_metrics()
            models.save_checkpoint(model, optimizer, self.path_last, model.epoch)
