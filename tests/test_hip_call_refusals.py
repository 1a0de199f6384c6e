"""What the C ABI refuses of a malformed call, for both kernel families.

``njode_plan_f32``, ``njode_forward_f32`` and ``njode_backward_f32`` are called through ``ctypes`` (as
``test_hip_buffer_bounds`` calls them) on one compiled shape (the demo shape) and one shape of the
shape-generic family, at B = 2, n_obs = 3, n_times = 2, K = 4, with ONE thing wrong per call: a null
argument, a negative size, a null batch or schedule array, a masked model without M (on a masked shape of
each family), get_loss without n_obs_ot, dropout_p outside [0, 1), a workspace one byte short,
NJODE_C_PLAN_READY without a plan.  Per call: the return code, the text of ``njode_last_error()``, and
that nothing was launched -- outputs, workspace and plan buffer keep the pattern they were filled with.
The well-formed call of every shape runs first and returns 0, so each refusal is the one fault's.

The expected (code, message) pairs are those of the library before the two families shared their call
front (njode_call.h); where the families differ (a plan needs neither M nor n_obs_ot in the generic
family, and names its buffer differently) the table says so.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_OBS, NT, K = 2, 3, 2, 4
OK, E_UNSUPPORTED, E_BADARG, E_WORKSPACE = 0, 1, 2, 3
TANH = 0
F_MASKED, F_RESIDUAL = 0x1, 0x4

# name: (family, d, H, d_out, n_hidden, width, flags)
SHAPES = {
    'compiled': ('compiled', 1, 10, 1, 2, 50, F_RESIDUAL),                       # build.CONFIGS[0], the demo shape
    'generic': ('generic', 3, 9, 3, 2, 33, F_RESIDUAL),
    'compiled_masked': ('compiled', 41, 41, 41, 2, 50, F_RESIDUAL | F_MASKED),   # build.CONFIGS[6]
    'generic_masked': ('generic', 7, 7, 7, 2, 21, F_RESIDUAL | F_MASKED),
}
NULL_ARG = (E_BADARG, 'null argument')
NEG = (E_BADARG, 'negative size')
BATCH_ARR = (E_BADARG, 'null batch array')
SCHED_ARR = (E_BADARG, 'null schedule array')


def cases(family, masked):
    """[(case, entry points it applies to, (code, message))]; '{short}' / '{need}': the byte counts."""
    every, calls = ('plan', 'forward', 'backward'), ('forward', 'backward')
    # (a generic plan reads neither M nor n_obs_ot and does not ask for them)
    plan_too = every if family == 'compiled' else calls
    out = [('dims=null', every, NULL_ARG), ('batch=null', every, NULL_ARG), ('sched=null', every, NULL_ARG),
           ('params=null', calls, NULL_ARG), ('ws=null', calls, NULL_ARG),
           ('ws=null', ('plan',), NULL_ARG if family == 'compiled' else (E_BADARG, 'null plan buffer')),
           ('batch_size=0', every, NEG), ('n_obs=-1', every, NEG), ('n_steps=-1', every, NEG), ('n_times=-1', every, NEG),
           ('start_X=null', every, BATCH_ARR), ('X=null', every, BATCH_ARR), ('obs_idx=null', every, BATCH_ARR)]
    out += [(f + '=null', every, SCHED_ARR) for f in ('step_dt', 'step_t', 'k_jump', 'time_f32', 'time_ptr')]
    if masked:
        out.append(('M=null', plan_too, (E_BADARG, 'masked model needs M')))
    out += [('n_obs_ot=null', plan_too, (E_BADARG, 'get_loss needs n_obs_ot')),
            ('dropout_p=-0.1', calls, (E_BADARG, 'dropout_p')), ('dropout_p=1.0', calls, (E_BADARG, 'dropout_p')),
            ('ws_short', calls, (E_WORKSPACE, 'workspace too small: {short} < {need}')),
            ('ws_short', ('plan',), (E_WORKSPACE, ('workspace' if family == 'compiled' else 'plan buffer')
                                     + ' too small: {short} < {need}')),
            ('plan_ready', calls, (E_BADARG, 'NJODE_C_PLAN_READY without NjodeBatch.plan'))]
    return out


class Setup:
    """A well-formed call of one shape and everything it points at."""

    def __init__(self, name):
        from njode_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.family, d, H, DO, nh, W, flags = SHAPES[name]
        self.masked = bool(flags & F_MASKED)
        self.dims = _lib.NjodeDims(d, H, DO, nh, W, TANH, flags)
        assert self.L.njode_supported(ctypes.byref(self.dims)) == 1
        info = 'd{}.h{}.o{}.nh{}.w{}.a{}.f{};'.format(d, H, DO, nh, W, TANH, flags)
        assert (info in _lib.build_info()) == (self.family == 'compiled'), name
        self.P = self.L.njode_param_count(ctypes.byref(self.dims))
        g = torch.Generator().manual_seed(d)
        rand = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
        self.t = dict(params=rand(self.P), start_X=rand(B, d), X=rand(N_OBS, d), M=torch.ones(N_OBS, d).cuda(),
                      obs_idx=torch.tensor([0, 1, 0], dtype=torch.int32).cuda(),
                      n_obs_ot=torch.tensor([2, 1], dtype=torch.int32).cuda(), grad_loss=torch.ones(1).cuda())
        # the schedule: four Euler steps of 0.25, jumps behind the second and the fourth (no tail)
        self.sched = dict(step_dt=np.full(K, 0.25, np.float32), step_t=np.arange(K, dtype=np.float32) * 0.25,
                          k_jump=np.array([2, 4], np.int32), time_f32=np.array([0.5, 1.0], np.float32),
                          time_ptr=np.array([0, 2, 3], np.int32))
        self.flags = _lib.C_TRAIN | _lib.C_GET_LOSS | _lib.C_SAVE_BWD
        need, pneed = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(self.L.njode_workspace_bytes(ctypes.byref(self.dims), B, N_OBS, NT, K, self.flags, ctypes.byref(need)))
        _lib.check(self.L.njode_plan_bytes(ctypes.byref(self.dims), B, N_OBS, NT, K, self.flags, ctypes.byref(pneed)))
        self.need = {'plan': pneed.value, 'forward': need.value, 'backward': need.value}
        self.out = dict(hT=torch.empty(B, H).cuda(), loss=torch.empty(1).cuda(), grad_params=torch.empty(self.P).cuda(),
                        ws=torch.empty(need.value, dtype=torch.uint8).cuda(),
                        plan=torch.empty(pneed.value, dtype=torch.uint8).cuda())
        self.stream = torch.cuda.current_stream().cuda_stream

    def fill(self):
        for k, v in self.out.items():
            v.view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()

    def untouched(self):
        torch.cuda.synchronize()
        return [k for k, v in self.out.items() if not bool((v.view(torch.uint8) == 0xA5).all())]

    def call(self, entry, case=None):
        """The return code of ``entry`` with ``case`` wrong (None: the well-formed call)."""
        lib, L, t = self.lib, self.L, self.t
        ptr = {k: v.data_ptr() for k, v in t.items()}
        ptr.update({k: v.ctypes.data for k, v in self.sched.items()})
        size = dict(batch_size=B, n_obs=N_OBS, n_steps=K, n_times=NT)
        ws = self.out['plan' if entry == 'plan' else 'ws'].data_ptr()
        ws_bytes, flags, dropout_p = self.need[entry], self.flags, 0.1
        null = set()
        if case == 'ws_short':
            ws_bytes -= 1
        elif case == 'plan_ready':
            flags |= lib.C_PLAN_READY
        elif case is not None:
            field, value = case.split('=')
            if value == 'null':
                null.add(field)
            elif field == 'dropout_p':
                dropout_p = float(value)
            else:
                size[field] = int(value)
        p = lambda k: None if k in null else ptr[k]
        cb = lib.NjodeBatch(size['batch_size'], size['n_obs'], p('start_X'), p('X'), p('M') if self.masked else None,
                            p('obs_idx'), p('n_obs_ot'), float(B), 0, None, None)
        cs = lib.NjodeSchedule(size['n_steps'], size['n_times'], p('step_dt'), p('step_t'), p('k_jump'),
                               p('time_f32'), p('time_ptr'))
        dims = None if 'dims' in null else ctypes.byref(self.dims)
        cb = None if 'batch' in null else ctypes.byref(cb)
        cs = None if 'sched' in null else ctypes.byref(cs)
        ws = None if 'ws' in null else ws
        if entry == 'plan':
            return L.njode_plan_f32(dims, cb, cs, flags, ws, ws_bytes, self.stream)
        common = (dims, p('params'), cb, cs, flags, 0.5, dropout_p, 7)
        if entry == 'forward':
            return L.njode_forward_f32(*common, self.out['hT'].data_ptr(), self.out['loss'].data_ptr(), None, None,
                                       ws, ws_bytes, self.stream)
        return L.njode_backward_f32(*common, ptr['grad_loss'], self.out['grad_params'].data_ptr(), ws, ws_bytes,
                                    self.stream)


@pytest.mark.parametrize('name', list(SHAPES))
def test_singly_malformed_calls_are_refused_before_anything_is_launched(name):
    s = Setup(name)
    # the well-formed calls: a plan into its own buffer, then the step on the workspace
    for entry in ('plan', 'forward', 'backward'):
        rc = s.call(entry)
        assert rc == OK, (entry, rc, s.L.njode_last_error().decode())
    torch.cuda.synchronize()
    assert np.isfinite(float(s.out['loss'])) and bool(torch.isfinite(s.out['grad_params']).all())
    errors, n = [], 0
    for case, entries, (code, msg) in cases(s.family, s.masked):
        for entry in entries:
            s.fill()
            rc = s.call(entry, case)
            text = s.L.njode_last_error().decode()
            want = msg.format(short=s.need[entry] - 1, need=s.need[entry])
            n += 1
            if (rc, text) != (code, want):
                errors.append('{} {}: returned ({}, {!r}), expected ({}, {!r})'.format(entry, case, rc, text, code, want))
            touched = s.untouched()
            if touched:
                errors.append('{} {}: refused, but wrote {}'.format(entry, case, touched))
    print('{}: {} refused calls'.format(name, n))
    assert not errors, '\n'.join(errors)
