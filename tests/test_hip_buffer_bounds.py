"""Every caller-owned buffer of the C ABI held to its stated size, on every kernel route.

The Python wrapper hands the library workspaces of ``1.25 need + 4096`` bytes and outputs from
``torch.empty``, which rounds every block up; a C caller allocates what ``include/njode_hip.h``
states.  Here the entry points are called through ``ctypes`` with every buffer carved out of a
guard-band arena (``tests/guarded.py``): exactly ``njode_workspace_bytes`` / ``njode_plan_bytes`` /
``njode_cond_exp_bytes`` bytes of workspace, outputs of exactly their stated shape, quiet NaNs
around the float inputs, valid-but-wrong indices around the integer inputs.  Per call:

1. the return code is 0 at exactly the stated sizes;
2. no guard byte before or behind any buffer (inputs included) changed;
3. every output is BIT FOR BIT the output of the same call made by the roomy Python wrapper in the
   same process with the same dropout seed;
4. the call repeated under the other phase of the workspace / plan / output pattern gives the same
   bits: nothing read from a guard, or from workspace the call did not write, reached a result.

Rows: the route table of ``test_hip_route_matrix`` (every compiled configuration on every route at
its own batch kind), the long schedules K = 512 / 4 096 / 4 070 dense, the record-budget
environments, and five shape-generic shapes whose sizes are no multiples of 4.  One child process
per environment (the switches are read once per process), one pass over its jobs; the route of
every row is confirmed by the kernel names of ``njode_profile_read``.  No oracle runs here.
The producer and the conditional expectation follow in-process at the end of the module.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import test_hip_route_matrix as RM
from guarded import Arena
from hip_util import exact_k_batch, hip_model, kernel_names
from njode_amd.build import CONFIGS
from test_hip_route_matrix import ENVS, check_names, job_batch, make_batch, model_cfg, routes

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
SEED, STEP = 5, 7          # options['dropout_seed'] and NJODE._step_counter of every call
GRAD_LOSS = 0.7            # upstream gradient of the autograd pair


def _w(n, act='tanh', layers=2):
    return tuple((n, act) for _ in range(layers))


def _gcfg(d, H, DO, ode, enc, dec, rnn=False, **options):
    options.setdefault('residual_enc_dec', True)
    return dict(input_size=d, hidden_size=H, output_size=DO, ode_nn=ode, readout_nn=dec, enc_nn=enc,
                use_rnn=rnn, bias=True, dropout_rate=0.0, options=options)


# shape-generic shapes (admitted by gen_envelope.restate_cfg): H, d, d_out no multiples of 4;
# name: (config, (B, K, observations per path), dropout)
GEN = {
    'g_d3_h9': (_gcfg(3, 9, 3, _w(33), _w(33), _w(33)), (17, 40, 4), 0.1),
    'g_rnn_d5_h10': (_gcfg(5, 10, 5, _w(50), _w(50), _w(50), rnn=True), (17, 40, 4), 0.1),
    # per_net: three different networks
    'g_pernet_d17_h34': (_gcfg(17, 34, 17, _w(48), _w(40, 'relu'), _w(72)), (17, 40, 4), 0.0),
    'g_masked_d7': (_gcfg(7, 7, 7, _w(21), _w(21), _w(21), masked=True), (19, 40, 4), 0.1),
    # output_size != input_size: prediction calls only
    'g_d3_h13_do7': (_gcfg(3, 13, 7, _w(30), _w(30), _w(30), residual_enc_dec=False), (17, 40, 4), 0.1),
}


def _gen_batch(name):
    cfg, (B, K, n_obs), _ = GEN[name]
    d = cfg['input_size']
    if cfg['options'].get('masked'):
        from njode_amd import synthetic_physionet
        b = synthetic_physionet.make_batch(batch_size=B, dim=d, n_grid=K, n_obs_range=(2, n_obs + 3), seed=B + d)
        return b, b['delta_t'], b['T']
    return exact_k_batch(B, K, obs_per_path=n_obs, seed=B * 7 + K + d, d=d)


def _setup(job):
    """(model config with the job's dropout, config for the initial parameters, batch, delta_t, T)."""
    if 'gen' in job:
        cfg0 = GEN[job['gen']][0]
        b, dt, T = _gen_batch(job['gen'])
        return dict(cfg0, dropout_rate=job['dropout']), cfg0, b, dt, T
    c = tuple(job['cfg'])
    b, dt, T = job_batch(job, c)
    return model_cfg(c, job['dropout']), model_cfg(c), b, dt, T


# ---- child side: one row -------------------------------------------------------------------------------
def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Row:
    """One model on one batch: the wrapper's calls and the same calls on guarded buffers."""

    def __init__(self, job):
        from njode_amd import _lib, models
        self.lib, self.L = _lib, _lib.lib()
        self.job = job
        cfg, cfg0, b, dt, T = _setup(job)
        torch.manual_seed(0)
        self.m = m = hip_model(cfg, models.NJODE(**cfg0).state_dict()).train()
        m.seed = SEED
        self.b, self.dt, self.T = b, dt, T
        self.T_tail = float(b['times'][-1]) + RM.TAIL_STEPS * dt
        self.M = b['M'].cuda().float().contiguous() if 'M' in b else None
        self.args = lambda T_: (b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), dt, T_,
                                b['start_X'].cuda(), b['n_obs_ot'].cuda().int())
        self.X = b['X'].cuda().float().contiguous()
        self.start_X = b['start_X'].cuda().float().contiguous()
        self.obs_idx = b['obs_idx'].cuda().int().contiguous()
        self.n_obs_ot = b['n_obs_ot'].cuda().int().contiguous()
        self.lock = bool(m.masked or m.use_rnn)      # the lockstep plan whatever the schedule
        self.has_loss = m.input_size == m.output_size
        self.errors, self.calls, self.buffers, self.names = [], 0, 0, {}
        self.stream = torch.cuda.current_stream().cuda_stream

    def err(self, *what):
        self.errors.append('{}: {}'.format(self.job['id'], ' '.join(str(w) for w in what)))

    # -- the structs of a call, as the wrapper builds them ------------------------------------------
    def structs(self, T, **kw):
        kw.setdefault('return_path', False), kw.setdefault('get_loss', True), kw.setdefault('until_T', False)
        m = self.m
        a = self.args(T)
        m._step_counter = STEP
        c = m._describe_call(
            a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], return_path=kw['return_path'],
            get_loss=kw['get_loss'], until_T=kw['until_T'], M=self.M, save_bwd=kw.get('save_bwd', False),
            rows_in_fwd=kw.get('rows_in_fwd', False))
        return dict(dims=c.dims, cb=c.batch, cs=c.sched, flags=c.flags, keep=c.keep, slot=c.slot_i, sizes=c.sizes,
                    get_loss=kw['get_loss'], n_rows=1 + c.sizes[3] + c.sizes[2])

    def release(self, S):
        torch.cuda.synchronize()
        self.m._ring.release_after(S['slot'], torch.cuda.current_stream())

    @property
    def seed(self):
        return (self.m.seed * 0x9E3779B97F4A7C15 + STEP) & 0xFFFFFFFFFFFFFFFF

    # -- one guarded step: [plan,] forward [, backward] on ONE arena -------------------------------
    def guarded(self, tag, S, phase, flags, want_hT=True, path=False, plan=None, backward=None,
                grad_loss=1.0, grad_hT=None, loss_batch=None):
        """Returns {output name: tensor} or None after a failed call.  ``plan``: None | 'inline' |
        'defer'; ``backward``: None | 'loss' (njode_backward_loss_f32) | 'plain' (njode_backward_f32)."""
        lib, L, m = self.lib, self.L, self.m
        B, n_obs, nt, K = S['sizes']
        H, DO, D, P = m.hidden_size, m.output_size, m.input_size, m._flat.numel()
        get_loss = bool(flags & lib.C_GET_LOSS)
        dims = S['dims']
        plan_flags = 0
        if plan:
            plan_flags = (flags & ~(lib.C_LOSS_IN_BWD | lib.C_ROWS_IN_FWD)) | (lib.C_NEED_HT if want_hT else 0)
            flags |= lib.C_PLAN_READY | (lib.C_NEED_HT if want_hT else 0)
        need, pneed = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = L.njode_workspace_bytes(ctypes.byref(dims), B, n_obs, nt, K, flags, ctypes.byref(need))
        if rc == 0 and plan:
            rc = L.njode_plan_bytes(ctypes.byref(dims), B, n_obs, nt, K, plan_flags, ctypes.byref(pneed))
        if rc:
            return self.err(tag, 'size query failed', rc, L.njode_last_error().decode())
        A = Arena('cuda', phase)
        A.add('params', 4 * P, 'nan32').add('start_X', 4 * B * D, 'nan32')
        if n_obs:
            A.add('X', 4 * n_obs * D, 'nan32').add('obs_idx', 4 * n_obs, 'index', modulo=min(B, 3))
            if self.M is not None:
                A.add('M', 4 * n_obs * D, 'nan32')
        if get_loss:
            A.add('n_obs_ot', 4 * B, 'index', base=1).add('loss', 4)
        if want_hT:
            A.add('hT', 4 * B * H)
        if path:
            A.add('path_h', 4 * S['n_rows'] * B * H).add('path_y', 4 * S['n_rows'] * B * DO)
        if backward:
            A.add('grad_loss', 4, 'nan32').add('grad_params', 4 * P)
        if grad_hT is not None:
            A.add('grad_hT', 4 * B * H, 'nan32')
        A.add('workspace', need.value)
        if plan:
            A.add('plan', pneed.value)
        A.build()
        self.buffers += len(A.specs)
        A.put('params', m._flat), A.put('start_X', self.start_X)
        if n_obs:
            A.put('X', self.X), A.put('obs_idx', self.obs_idx)
            if self.M is not None:
                A.put('M', self.M)
        if get_loss:
            A.put('n_obs_ot', self.n_obs_ot)
        if backward:
            A.put('grad_loss', torch.tensor([grad_loss], dtype=torch.float32))
        if grad_hT is not None:
            A.put('grad_hT', grad_hT)
        p = lambda name: A.ptr(name) if name in A.where else None
        cb0 = S['cb']
        cb = lib.NjodeBatch(B, n_obs, p('start_X'), p('X'), p('M'), p('obs_idx'), p('n_obs_ot'),
                            cb0.loss_batch_size if loss_batch is None else loss_batch, cb0.path_id_offset,
                            p('plan'), None)
        cs = S['cs']
        common = (float(m.weight), float(m.dropout_rate), self.seed)

        def done(what, rc):
            self.calls += 1
            if rc:
                self.err(tag, what, 'returned', rc, L.njode_last_error().decode())
            trips = A.check()
            if trips:
                self.err(tag, what, 'phase', phase, 'wrote outside its buffers:', trips)
            return rc == 0

        if plan:
            rc = L.njode_plan_f32(ctypes.byref(dims), ctypes.byref(cb), ctypes.byref(cs),
                                  plan_flags | (lib.C_PLAN_DEFER if plan == 'defer' else 0), p('plan'),
                                  pneed.value, self.stream)
            if not done('njode_plan_f32', rc):
                return None
        rc = L.njode_forward_f32(ctypes.byref(dims), p('params'), ctypes.byref(cb), ctypes.byref(cs), flags,
                                 *common, p('hT'), p('loss'), p('path_h'), p('path_y'), p('workspace'),
                                 need.value, self.stream)
        if not done('njode_forward_f32', rc):
            L.njode_plan_flush()
            return None
        if backward:
            cb.grad_hT = p('grad_hT')
            if backward == 'loss':
                rc = L.njode_backward_loss_f32(ctypes.byref(dims), p('params'), ctypes.byref(cb), ctypes.byref(cs),
                                               flags, *common, p('grad_loss'), p('grad_params'), p('loss'),
                                               p('workspace'), need.value, self.stream)
            else:
                rc = L.njode_backward_f32(ctypes.byref(dims), p('params'), ctypes.byref(cb), ctypes.byref(cs),
                                          flags, *common, p('grad_loss'), p('grad_params'), p('workspace'),
                                          need.value, self.stream)
            if not done('njode_backward', rc):
                return None
        out = {}
        for name in ('loss', 'hT', 'path_h', 'path_y', 'grad_params'):
            if name in A.where:
                out[name] = A.view(name, torch.float32).clone()
        # the inputs themselves are as they were put
        if not torch.equal(A.view('params', torch.float32).view(torch.int32), m._flat.view(torch.int32)):
            self.err(tag, 'params were modified')
        return out

    def compare(self, tag, got, ref):
        """Both phases of a guarded step against the wrapper's tensors {name: tensor}."""
        for phase, g in enumerate(got):
            if g is None:
                continue
            for name, r in ref.items():
                if r is None:
                    continue
                if not _bits_equal(g[name].reshape(-1), r.detach().reshape(-1).float()):
                    d = (g[name].reshape(-1).double() - r.detach().reshape(-1).double()).abs().max().item()
                    self.err(tag, name, 'phase', phase, 'differs from the wrapper call: max abs', d)

    def both(self, tag, S, flags, ref, **kw):
        got = [self.guarded(tag, S, phase, flags, **kw) for phase in (0, 1)]
        self.compare(tag, got, ref)

    # -- the calls of a row ------------------------------------------------------------------------------
    def run(self):
        lib, m = self.lib, self.m
        if self.has_loss:
            self.fused_and_planned()
            self.autograd_pair()
            if self.lock:
                self.through_hT()
        self.predict()
        return self

    def fused_and_planned(self):
        lib, m = self.lib, self.m
        a = self.args(self.T)
        # the wrapper: the fused step; the same from a prefetched plan; hT of the segment plan from
        # the training forward (loss_and_grad does not ask for it)
        m._step_counter = STEP
        (hT, loss), names = kernel_names(lambda: m.loss_and_grad(*a, M=self.M))
        self.names['fused'] = names
        ref = {'loss': loss.clone().reshape(1), 'grad_params': m.flat_grad().clone(), 'hT': hT}
        m._step_counter = STEP
        m._plans.clear()
        m.prefetch_plan(*a, M=self.M, need_hT=self.lock)
        _, loss_p = m.loss_and_grad(*a, M=self.M)
        ref_p = {'loss': loss_p.clone().reshape(1), 'grad_params': m.flat_grad().clone()}
        S = self.structs(self.T, save_bwd=True)
        flags = S['flags'] | lib.C_LOSS_IN_BWD
        assert flags & lib.C_TRAIN and flags & lib.C_SCHED_KNOWN
        # a. the fused step, guarded; its kernel names are the route's
        got0, gnames = kernel_names(lambda: self.guarded('fused', S, 0, flags, want_hT=self.lock, backward='loss'))
        self.names['guarded'] = gnames
        self.compare('fused', [got0, self.guarded('fused', S, 1, flags, want_hT=self.lock, backward='loss')], ref)
        if not self.lock:
            m._step_counter = STEP
            hT_fwd = m(*a, M=self.M)[0].detach().clone()      # (a saving forward, as the fused step's is)
            self.both('fused+hT', S, flags, dict(ref, hT=hT_fwd), want_hT=True, backward='loss')
        # b. the same step from a plan built ahead into a buffer of exactly njode_plan_bytes
        self.both('plan', S, flags, ref_p, want_hT=self.lock, backward='loss', plan='inline')
        if m.plan_defer_ok(S['sizes'][1]):
            self.both('plan_defer', S, flags, ref_p, want_hT=self.lock, backward='loss', plan='defer')
        self.release(S)

    def autograd_pair(self):
        lib, m = self.lib, self.m
        a = self.args(self.T)
        m._step_counter = STEP
        m.zero_grad()
        hT, loss = m(*a, M=self.M)
        (GRAD_LOSS * loss).backward()
        grad = torch.zeros_like(m._flat)
        for (off, n, _), p in zip(m._param_slices, m._flat_params):
            grad[off:off + n] = p.grad.reshape(-1)
        ref = {'loss': loss.detach().clone().reshape(1), 'hT': hT.detach().clone(), 'grad_params': grad}
        m.zero_grad()
        S = self.structs(self.T, save_bwd=True, rows_in_fwd=True)
        assert S['flags'] & lib.C_ROWS_IN_FWD
        self.both('autograd', S, S['flags'], ref, want_hT=True, backward='plain', grad_loss=GRAD_LOSS)
        self.release(S)

    def through_hT(self):
        """Lockstep rows: the backward that starts from an upstream gradient of hT, through an until_T tail
        (the wrapper's ``_grad_through_hT``: loss switched off by loss_batch_size = inf)."""
        lib, m = self.lib, self.m
        a = self.args(self.T_tail)
        B, H = self.start_X.shape[0], m.hidden_size
        gh = RM.c_hT(B, H).cuda().contiguous()
        m._step_counter = STEP
        call = m._arm_call(m._describe_call(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], until_T=True,
                                            M=self.M, save_bwd=True))
        slot = call.slot_i
        try:
            ref_grad = m._grad_through_hT(call, gh).clone()
            ref = {'grad_params': ref_grad, 'hT': m._last_hT_replay.clone()}
        finally:
            m._release_ws(call)
            torch.cuda.synchronize()
            m._ring.release_after(slot, torch.cuda.current_stream())
        S = self.structs(self.T_tail, until_T=True, save_bwd=True)
        assert S['flags'] & lib.C_SCHED_TAIL
        flags = ((S['flags'] & (lib.C_TRAIN | lib.C_SCHED_KNOWN | lib.C_SCHED_TAIL))
                 | lib.C_GET_LOSS | lib.C_SAVE_BWD | lib.C_GEN_LOCKSTEP)
        self.both('grad_hT', S, flags, ref, want_hT=True, backward='plain', grad_hT=gh, loss_batch=float('inf'))
        self.release(S)

    def predict(self):
        lib, m = self.lib, self.m
        m.eval()
        try:
            for get_loss in ((False, True) if self.has_loss else (False,)):
                until = self.lock
                T = self.T_tail if until else self.T
                a = self.args(T)
                with torch.no_grad():
                    out, names = kernel_names(lambda: m(*a, M=self.M, return_path=True, get_loss=get_loss,
                                                        until_T=until))
                self.names['predict'] = names
                ref = {'hT': out[0], 'path_h': out[3], 'path_y': out[4]}
                if get_loss:
                    ref['loss'] = out[1].reshape(1)
                S = self.structs(T, return_path=True, get_loss=get_loss, until_T=until)
                assert not S['flags'] & lib.C_TRAIN and tuple(out[3].shape)[0] == S['n_rows']
                self.both('predict' + ('+loss' if get_loss else ''), S, S['flags'], ref, want_hT=True, path=True)
                self.release(S)
        finally:
            m.train()


def _adam_rows(errors):
    """njode_adam_step_f32 on the demo model's own P (no multiple of 256) and on n = 1, 255, 257."""
    from njode_amd import _lib, models
    L = _lib.lib()
    torch.manual_seed(0)
    m = hip_model(model_cfg(CONFIGS[0])).train()
    P = m.flat_parameters().numel()
    assert P % 256
    calls = buffers = 0
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0005)
    for n in (P, 1, 255, 257):
        g = torch.Generator().manual_seed(n)
        p0, gr, m0 = (torch.randn(n, generator=g).cuda() for _ in range(3))
        v0 = torch.rand(n, generator=g).cuda()
        if n == P:      # the wrapper's own call: FusedAdam.step on the model
            opt = models.FusedAdam(m, lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4])
            m.flat_parameters().copy_(p0), m.flat_grad().copy_(gr), opt.exp_avg.copy_(m0), opt.exp_avg_sq.copy_(v0)
            opt.step_count = 2
            opt.step()
            ref = [m.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
        else:           # (FusedAdam only steps whole models: the same ctypes call on torch's own tensors)
            ref = [p0.clone(), m0.clone(), v0.clone()]
            _lib.check(L.njode_adam_step_f32(ref[0].data_ptr(), gr.data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(),
                                             n, *hyper, 3, 1.0, torch.cuda.current_stream().cuda_stream))
        for phase in (0, 1):
            A = Arena('cuda', phase)
            A.add('params', 4 * n).add('grad', 4 * n, 'nan32').add('exp_avg', 4 * n).add('exp_avg_sq', 4 * n).build()
            A.put('params', p0), A.put('grad', gr), A.put('exp_avg', m0), A.put('exp_avg_sq', v0)
            rc = L.njode_adam_step_f32(A.ptr('params'), A.ptr('grad'), A.ptr('exp_avg'), A.ptr('exp_avg_sq'), n,
                                       *hyper, 3, 1.0, torch.cuda.current_stream().cuda_stream)
            calls, buffers = calls + 1, buffers + 4
            trips = A.check()
            if rc or trips:
                errors.append('adam n={} phase {}: rc {} guards {}'.format(n, phase, rc, trips))
            for name, r in zip(('params', 'exp_avg', 'exp_avg_sq'), ref):
                if not _bits_equal(A.view(name, torch.float32), r):
                    errors.append('adam n={} phase {}: {} differs from the wrapper call'.format(n, phase, name))
            if not _bits_equal(A.view('grad', torch.float32), gr):
                errors.append('adam n={}: the gradient was modified'.format(n))
    return calls, buffers


def _child(jobs, out_path):
    res = {'errors': [], 'rows': {}, 'calls': 0, 'buffers': 0}
    for job in jobs:
        if job.get('adam'):
            c, b = _adam_rows(res['errors'])
            res['calls'] += c
            res['buffers'] += b
            continue
        # (the shape-generic kernels' plan switch is read per step, by the wrapper)
        os.environ.pop('NJODE_GEN_PLAN', None)
        if job.get('gen_plan') == 'lock':
            os.environ['NJODE_GEN_PLAN'] = 'lock'
        row = Row(job).run()
        res['errors'] += row.errors
        res['calls'] += row.calls
        res['buffers'] += row.buffers
        res['rows'][job['id']] = {'names': row.names, 'n_obs': int(row.b['time_ptr'][-1]),
                                  'B': int(row.start_X.shape[0])}
        del row
        torch.cuda.empty_cache()
    with open(out_path, 'w') as f:
        json.dump(res, f)


_SNIPPET = r'''
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_hip_buffer_bounds as T
T._child(json.load(open({jobs!r})), {out!r})
'''


DEAD = []      # children that did not end cleanly


def _no_dead_child():
    assert not DEAD, 'a child process of the route rows died {}: nothing more runs on the GPU'.format(DEAD)


def run_child(tmp_path, tag, env, jobs, timeout=600):
    out = tmp_path / tag
    out.mkdir()
    with open(out / 'jobs.json', 'w') as f:
        json.dump(jobs, f)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, '-c', _SNIPPET.format(tests=TESTS, repo=REPO, jobs=str(out / 'jobs.json'),
                                                                   out=str(out / 'res.json'))],
                           env=dict(os.environ, **env), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        DEAD.append((tag, 'timeout'))
        raise
    # (a child that died -- a fault, an abort -- ends the test here, and the tests behind it in this
    # module fail before they touch the GPU: nothing more is started on it)
    if p.returncode != 0:
        DEAD.append((tag, p.returncode))
    assert p.returncode == 0, (tag, p.returncode, p.stdout[-4000:])
    with open(out / 'res.json') as f:
        res = json.load(f)
    print('child {}: {} rows, {} calls, {} guarded buffers, {:.1f} s'.format(tag, len(res['rows']), res['calls'],
                                                                             res['buffers'], time.time() - t0))
    return res


# ---- parent side: the table -------------------------------------------------------------------------------
def _drop(c):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    return 0.1 if nh > 0 and W <= 64 else 0.0      # (where the kernels draw masks: hidden layers up to 64 wide)


GEN_SEG = ['k_gseg_ode_fwd']
GEN_LOCK = ['k_gen_fwd']


def table():
    """({environment tag: (environment, [job])}, {job id: (kernels that must run, must not run)})."""
    envs = {tag: (dict(env), []) for tag, env in ENVS.items()}
    expect = {}
    for i, c in enumerate(CONFIGS):
        for name, env, kind, must, must_not in routes(c):
            jid = 'c{}_{}'.format(i, name)
            envs[env][1].append({'id': jid, 'cfg': list(c), 'batch': kind, 'dropout': _drop(c)})
            expect[jid] = (must, must_not)
    # the long schedules (test_long_schedules_against_float64)
    for kind, must in (('K512', RM.ITEMS), ('K4096', RM.ONE_WAVE), ('K4070dense', RM.MIXED)):
        envs['default'][1].append({'id': kind, 'cfg': list(RM.DEMO), 'batch': kind, 'dropout': 0.1})
        expect[kind] = (must, [n for n in RM.ITEMS + RM.MIXED + RM.ONE_WAVE if n not in must])
    # the shape-generic kernels, on both of their plans where the shape has both
    for name, (cfg, _, drop) in GEN.items():
        envs['default'][1].append({'id': name, 'gen': name, 'dropout': drop})
        lock = cfg['options'].get('masked') or cfg['use_rnn'] or cfg['input_size'] != cfg['output_size']
        expect[name] = (GEN_LOCK if lock else GEN_SEG, list(RM.ITEMS + RM.MIXED + RM.ONE_WAVE))
        if not lock:
            envs['default'][1].append({'id': name + '_lock', 'gen': name, 'dropout': drop, 'gen_plan': 'lock'})
            expect[name + '_lock'] = (GEN_LOCK, GEN_SEG)
    envs['default'][1].append({'id': 'adam', 'adam': True})
    # the record budgets (test_record_budget_routes)
    mid, tiny = RM._budgets()
    demo = {'cfg': list(RM.DEMO), 'batch': 'small', 'dropout': 0.1}
    physio = {'cfg': list(RM.PHYSIO), 'batch': 'physio', 'dropout': 0.1}
    gen72 = {'cfg': list(RM.GENERIC72), 'batch': 'physio', 'dropout': 0.0}
    budget = {
        'mid': ({'NJODE_REC_BUDGET_GB': repr(mid)},
                {'demo': (RM.ITEMS + ['k_ode_dw_pairs_mfma'], ['k_ode_dw_stored*']),
                 'physio': (['k_paths_fwd_chain', 'k_ode_dw_pairs_mfma'], ['k_ode_dw_stored*'])}),
        'tiny': ({'NJODE_REC_BUDGET_GB': repr(tiny)},
                 {'demo': (RM.MIXED, RM.ITEMS), 'physio': (['k_paths_fwd_mfma'], ['k_paths_fwd_chain']),
                  'gen72': (['k_gen_fwd', 'k_gen_bwd', 'k_gen_dw'], ['k_gseg_ode_fwd', 'k_paths_fwd_mfma'])}),
        'tiny_tiles': ({'NJODE_REC_BUDGET_GB': repr(tiny), 'NJODE_SEG_CHAIN_MAX': '0', 'NJODE_CHAIN_MAX': '0',
                        'NJODE_LOCK4_PT': '16', 'NJODE_GEN_PT': '16'},
                       {'demo': (RM.MIXED, RM.ITEMS), 'physio': (['k_paths_fwd_mfma'], ['k_paths_fwd_chain']),
                        'gen72': (['k_gen_fwd', 'k_gen_bwd', 'k_gen_dw'], ['k_gseg_ode_fwd', 'k_paths_fwd_mfma'])}),
    }
    for tag, (env, rows) in budget.items():
        jobs = []
        for short, (must, must_not) in rows.items():
            jid = 'budget_{}_{}'.format(tag, short)
            jobs.append(dict({'demo': demo, 'physio': physio, 'gen72': gen72}[short], id=jid))
            expect[jid] = (must, must_not)
        envs['budget_' + tag] = (env, jobs)
    return envs, expect


def test_every_route_stays_inside_buffers_of_exactly_the_stated_size(tmp_path):
    t0 = time.time()
    envs, expect = table()
    errors, rows, calls, buffers = [], {}, 0, 0
    for tag, (env, jobs) in envs.items():
        _no_dead_child()
        res = run_child(tmp_path, tag, env, jobs)
        errors += res['errors']
        rows.update(res['rows'])
        calls += res['calls']
        buffers += res['buffers']
    # every row ran the route it stands for: the wrapper's fused step and the guarded one alike
    for jid, (must, must_not) in expect.items():
        info = rows[jid]
        try:
            for key in ('fused', 'guarded'):
                if key in info['names']:
                    check_names('{} ({})'.format(jid, key), info['names'][key], must, must_not)
            if 'fused' not in info['names']:      # a shape without a loss: its prediction call
                check_names(jid + ' (predict)', info['names']['predict'], must, must_not)
            if 'batch' in (job := next(j for _, js in envs.values() for j in js if j['id'] == jid)):
                RM.check_sizes(job['batch'], info['n_obs'], info['B'])
        except AssertionError as e:
            errors.append('{}: {}'.format(jid, e))
    print('buffer bounds: {} rows, {} guarded calls, {} guarded buffers, {:.1f} s'.format(
        len(rows), calls, buffers, time.time() - t0))
    assert not errors, '\n'.join(errors)


# ---- the producer and the conditional expectation (include/njode_producer.h) --------------------------
MODELS = ('BlackScholes', 'OrnsteinUhlenbeck', 'Heston')
PROD_SIZES = [(N, dim, S) for N in (1, 37, 65) for dim in (1, 3) for S in (7, 100)]
COUNTS = {'calls': 0, 'buffers': 0}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(A, name):
    return ctypes.c_void_p(A.ptr(name)) if name in A.where and A.nbytes(name) else ctypes.c_void_p(0)


def _finish(errors, tag, what, phase, rc, A, outputs):
    """Return code, guards and the bits of ``outputs`` {buffer: the wrapper's tensor} of one call."""
    COUNTS['calls'] += 1
    trips = A.check()
    if rc or trips:
        errors.append('{} {} phase {}: rc {} guards {}'.format(tag, what, phase, rc, trips))
    for name, ref in outputs.items():
        got = A.view(name, ref.dtype)
        if not torch.equal(got.view(torch.uint8), ref.contiguous().reshape(-1).view(torch.uint8)):
            errors.append('{} {} phase {}: {} differs from the wrapper call'.format(tag, what, phase, name))


def _producer_case(name, N, dim, S, errors):
    from njode_amd import _lib, data_utils, device_data
    from njode_amd.schedule import cond_exp_clock
    L = _lib.lib()
    tag = '{} N={} dim={} S={}'.format(name, N, dim, S)
    hp = dict(data_utils.hyperparam_default, nb_paths=N, nb_steps=S, S0=[1.0] * dim if dim > 1 else 1, obs_perc=0.4)
    seed = 3 + N + S
    # the wrapper's calls
    ds = device_data.DeviceDataset.generate(name, hp, seed=seed)
    funcs = ('power-2',) if dim == 1 else ()
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(N)).int().cuda()
    batch = ds.collate(idx, funcs)
    plain = ds.collate(idx, ()) if funcs else batch      # (lifted inputs have no conditional expectation)
    n_obs, width = int(batch['time_ptr'][-1]), dim * (1 + len(funcs))
    powers = device_data.parse_powers(funcs)
    pw = (ctypes.c_int32 * max(len(powers), 1))(*powers)
    sde = device_data.sde_struct(name, hp, dim)
    dt, T = ds.metadata['dt'], hp['maturity']
    ce = None
    if n_obs:
        clock = cond_exp_clock(plain['times'], dt, T)
        K, nt = clock.n_steps, clock.n_times
        n_t = 1 + K + nt
        pred = torch.randn((n_t, N, dim), generator=torch.Generator().manual_seed(S)).cuda()
        _, path_y, opt_loss, sq_diff = device_data.cond_exp(
            ds.metadata, plain['times'], plain['time_ptr'], plain['X'], plain['obs_idx'], dt, T, plain['start_X'],
            plain['n_obs_ot'], pred=pred, want_path=True, want_loss=True)
        ce = (clock, K, nt, n_t, pred, path_y, opt_loss.reshape(1).clone(), sq_diff.reshape(1).clone())
    for phase in (0, 1):
        # generation: outputs only
        A = Arena('cuda', phase)
        A.add('paths', 8 * (S + 1) * dim * N).add('observed', (S + 1) * N).add('nb_obs', 4 * N).build()
        COUNTS['buffers'] += 3
        rc = L.njode_generate_paths(ctypes.byref(sde), ctypes.c_uint64(seed), None, _vp(A, 'paths'), _stream())
        _finish(errors, tag, 'generate_paths', phase, rc, A, {'paths': ds.paths_tm})
        rc = L.njode_sample_observations(N, S, float(hp['obs_perc']), ctypes.c_uint64(seed), None,
                                         _vp(A, 'observed'), _vp(A, 'nb_obs'), _stream())
        _finish(errors, tag, 'sample_observations', phase, rc, A, {'observed': ds.observed_tm, 'nb_obs': ds.nb_obs})
        # collate: the dataset and the rows are inputs now
        A = Arena('cuda', phase)
        A.add('paths', 8 * (S + 1) * dim * N, 'nan64').add('observed', (S + 1) * N, 'index', modulo=2)
        A.add('nb_obs', 4 * N, 'index').add('idx', 4 * N, 'index', modulo=min(N, 3))
        A.add('counts', 4 * S).add('n_obs_ot', 4 * N).add('start_X', 4 * N * width)
        A.add('X', 4 * n_obs * width).add('obs_idx', 4 * n_obs).build()
        COUNTS['buffers'] += 9
        A.put('paths', ds.paths_tm), A.put('observed', ds.observed_tm), A.put('nb_obs', ds.nb_obs), A.put('idx', idx)
        rc = L.njode_collate_count(_vp(A, 'observed'), _vp(A, 'nb_obs'), N, S, _vp(A, 'idx'), N, _vp(A, 'counts'),
                                   _vp(A, 'n_obs_ot'), _stream())
        _finish(errors, tag, 'collate_count', phase, rc, A, {'n_obs_ot': batch['n_obs_ot']})
        times, time_ptr = device_data.times_from_counts(A.view('counts', torch.int32).cpu().numpy(), dt)
        if not (np.array_equal(times, batch['times']) and np.array_equal(time_ptr, batch['time_ptr'])):
            errors.append('{} collate_count phase {}: counts differ from the wrapper call'.format(tag, phase))
            continue
        rc = L.njode_collate_fill(_vp(A, 'paths'), _vp(A, 'observed'), N, dim, S, _vp(A, 'idx'), N, _vp(A, 'counts'),
                                  pw, len(powers), _vp(A, 'start_X'), _vp(A, 'X'), _vp(A, 'obs_idx'), _stream())
        _finish(errors, tag, 'collate_fill', phase, rc, A,
                {'start_X': batch['start_X'], 'X': batch['X'], 'obs_idx': batch['obs_idx']})
        if ce is None:
            continue
        # the conditional expectation: a workspace of exactly njode_cond_exp_bytes
        clock, K, nt, n_t, pred, path_y, opt_loss, sq_diff = ce
        need = ctypes.c_size_t(0)
        _lib.check(L.njode_cond_exp_bytes(N, n_obs, nt, K, dim, ctypes.byref(need)))
        A = Arena('cuda', phase)
        A.add('start_X', 4 * N * dim, 'nan32').add('X', 4 * n_obs * dim, 'nan32')
        A.add('obs_idx', 4 * n_obs, 'index', modulo=min(N, 3)).add('n_obs_ot', 4 * N, 'index', base=1)
        A.add('pred', 4 * n_t * N * dim, 'nan32').add('path_y', 8 * n_t * N * dim).add('opt_loss', 8)
        A.add('sq_diff', 8).add('ws', need.value).build()
        COUNTS['buffers'] += 9
        A.put('start_X', plain['start_X']), A.put('X', plain['X']), A.put('obs_idx', plain['obs_idx'])
        A.put('n_obs_ot', plain['n_obs_ot']), A.put('pred', pred)
        host = [np.ascontiguousarray(clock.step_dt, dtype=np.float64), np.ascontiguousarray(clock.step_t, dtype=np.float64),
                np.ascontiguousarray(clock.k_jump, dtype=np.int32), np.ascontiguousarray(plain['time_ptr'], dtype=np.int32)]
        sched = _lib.NjodeCondExpSchedule(K, nt, *[h.ctypes.data for h in host])
        cb = _lib.NjodeBatch(N, n_obs, A.ptr('start_X'), A.ptr('X'), None, A.ptr('obs_idx'), A.ptr('n_obs_ot'),
                             float(N), 0, None)
        rc = L.njode_cond_exp_f64(ctypes.byref(sde), ctypes.byref(cb), ctypes.byref(sched), 0.5, _vp(A, 'pred'),
                                  _vp(A, 'path_y'), _vp(A, 'opt_loss'), _vp(A, 'sq_diff'),
                                  ctypes.c_void_p(A.ptr('ws')), need.value, _stream())
        _finish(errors, tag, 'cond_exp', phase, rc, A, {'path_y': path_y, 'opt_loss': opt_loss, 'sq_diff': sq_diff})
        del host


@pytest.mark.parametrize('name', MODELS)
def test_producer_and_cond_exp_stay_inside_their_buffers(name):
    _no_dead_child()
    errors = []
    before = dict(COUNTS)
    for N, dim, S in PROD_SIZES:
        _producer_case(name, N, dim, S, errors)
    print('{}: {} guarded calls, {} guarded buffers'.format(name, COUNTS['calls'] - before['calls'],
                                                           COUNTS['buffers'] - before['buffers']))
    assert not errors, '\n'.join(errors)


def test_philox_stays_inside_its_buffers():
    _no_dead_child()
    from njode_amd import _lib
    L = _lib.lib()
    errors = []
    for n in (1, 37, 65):
        g = torch.Generator().manual_seed(n)
        ctr = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 4), generator=g, dtype=torch.int64).int().cuda()
        key = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 2), generator=g, dtype=torch.int64).int().cuda()
        ref = torch.empty((n, 4), dtype=torch.int32, device='cuda')
        _lib.check(L.njode_philox4x32_10(n, ctr.data_ptr(), key.data_ptr(), ref.data_ptr(), _stream()))
        for phase in (0, 1):
            A = Arena('cuda', phase)
            A.add('ctr', 16 * n, 'index').add('key', 8 * n, 'index').add('out', 16 * n).build()
            A.put('ctr', ctr), A.put('key', key)
            rc = L.njode_philox4x32_10(n, _vp(A, 'ctr'), _vp(A, 'key'), _vp(A, 'out'), _stream())
            _finish(errors, 'philox n={}'.format(n), 'philox4x32_10', phase, rc, A, {'out': ref})
    assert not errors, '\n'.join(errors)
