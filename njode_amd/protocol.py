"""
The real-data evaluation protocols on the GPU (C ABI: include/njode_protocol.h): which rows of a
prediction path answer a list of held-out times, and the masked squared errors of the prediction
at those rows.  Thin wrappers in the style of ``device_data.cond_exp``: tensors stay on the
device, nothing here waits for it, the workspace is allocated at exactly the size the library
states.  ``physionet_eval.evaluate_model_device`` and ``climate_eval.evaluate_model_device`` are
built on them.

No CPU fallback: everything here calls into ``libnjode_hip.so``; the host routes are
``physionet_eval.get_comparison_times_ind`` and ``climate_eval.extract_from_path``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import stream_arg as _stream

RULES = {'closest': _lib.ROWS_CLOSEST, 'first_nearest': _lib.ROWS_FIRST_NEAREST}


def _need_cuda(**tensors):
    dev = None
    for name, t in tensors.items():
        if not torch.is_tensor(t) or t.device.type != 'cuda':
            raise ValueError('{} must be a device tensor (the host routes are physionet_eval.'
                             'evaluate_model and climate_eval.evaluate_model)'.format(name))
        if dev is not None and t.device != dev:
            raise ValueError('{} is on {}, not on {}'.format(name, t.device, dev))
        dev = t.device
    return dev


def score_bytes(n_rows, n_query, B, dim):
    """``njode_protocol_bytes``: the workspace of one ``score`` call of these sizes."""
    need = C.c_size_t(0)
    _lib.check(_lib.lib().njode_protocol_bytes(int(n_rows), int(n_query), int(B), int(dim),
                                               C.byref(need)))
    return need.value


def rows(path_t, query, rule):
    """``njode_protocol_rows``: int32 device tensor ``[n_query]`` of the rows of ``path_t``
    (float64 device ``[n_rows]``, non-decreasing) that answer ``query`` (float64 device
    ``[n_query]``).  ``rule``: ``'closest'`` -- ``physionet_eval.get_comparison_times_ind`` -- or
    ``'first_nearest'`` -- the rows ``climate_eval.extract_from_path`` selects, for a ``path_t``
    already rounded and cast through float32."""
    if rule not in RULES:
        raise ValueError('rule must be one of {}'.format(sorted(RULES)))
    dev = _need_cuda(path_t=path_t, query=query)
    if path_t.dtype != torch.float64 or query.dtype != torch.float64 or path_t.dim() != 1 \
            or query.dim() != 1:
        raise ValueError('path_t and query must be 1-d float64 tensors')
    path_t, query = path_t.contiguous(), query.contiguous()
    out = torch.empty(query.numel(), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().njode_protocol_rows(
            path_t.data_ptr(), path_t.numel(), query.data_ptr(), query.numel(), RULES[rule],
            out.data_ptr(), _stream(dev)))
    return out


def score(pred, rows, vals=None, mask=None, X_val=None, M_val=None, index_val=None, out=None,
          accumulate=False):
    """``njode_protocol_score_f32``: ``out`` (float64 device ``[4]``, made here unless given) =
    ``[sq_sum, n_obs, attr_mse, 0]`` of ``pred`` (fp32 device ``[n_rows, B, dim]``, the model's
    ``path_y``) at ``rows`` (int32 device) against one target layout:

    * dense (PhysioNet): ``vals``, ``mask`` fp32 ``[B, T2, dim]``, ``rows [T2]``;
    * sparse (climate): ``X_val``, ``M_val`` fp32 ``[L, dim]``, ``rows [L]``, ``index_val`` int32
      ``[L]`` with entries in ``[0, B)`` (not checked here: a check would cost a host wait).

    ``accumulate``: add to what ``out`` holds.  ``ValueError``, before anything is launched: CPU
    tensors, both or neither layout, shapes that disagree, other dtypes."""
    dense = vals is not None or mask is not None
    sparse = X_val is not None or M_val is not None or index_val is not None
    if dense == sparse:
        raise ValueError('exactly one target layout: vals / mask or X_val / M_val / index_val')
    if dense:
        named = dict(pred=pred, rows=rows, vals=vals, mask=mask)
    else:
        named = dict(pred=pred, rows=rows, X_val=X_val, M_val=M_val, index_val=index_val)
    if any(v is None for v in named.values()):
        raise ValueError('half a target layout: {} missing'.format(
            [k for k, v in named.items() if v is None]))
    if out is not None:
        named['out'] = out
    dev = _need_cuda(**named)
    if pred.dim() != 3 or pred.dtype != torch.float32:
        raise ValueError('pred must be fp32 [n_rows, B, dim]')
    n_rows, B, dim = (int(s) for s in pred.shape)
    if rows.dim() != 1 or rows.dtype != torch.int32:
        raise ValueError('rows must be a 1-d int32 tensor')
    nq = rows.numel()
    if dense:
        for name in ('vals', 'mask'):
            t = named[name]
            if t.dtype != torch.float32 or tuple(t.shape) != (B, nq, dim):
                raise ValueError('{} must be fp32 [{}, {}, {}], not {} {}'.format(
                    name, B, nq, dim, t.dtype, tuple(t.shape)))
    else:
        for name in ('X_val', 'M_val'):
            t = named[name]
            if t.dtype != torch.float32 or tuple(t.shape) != (nq, dim):
                raise ValueError('{} must be fp32 [{}, {}], not {} {}'.format(
                    name, nq, dim, t.dtype, tuple(t.shape)))
        if index_val.dtype != torch.int32 or tuple(index_val.shape) != (nq,):
            raise ValueError('index_val must be int32 [{}]'.format(nq))
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs the out to add to')
        out = torch.empty(4, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (4,) or not out.is_contiguous():
        raise ValueError('out must be a contiguous float64 [4] tensor')
    keep = {k: v.contiguous() for k, v in named.items() if k != 'out'}
    p = lambda k: keep[k].data_ptr() if k in keep else None
    job = _lib.NjodeProtocolJob(p('pred'), n_rows, B, dim, nq, p('rows'), p('vals'), p('mask'),
                                p('X_val'), p('M_val'), p('index_val'))
    need = score_bytes(n_rows, nq, B, dim)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().njode_protocol_score_f32(
            C.byref(job), out.data_ptr(), int(bool(accumulate)), ws.data_ptr(), need, _stream(dev)))
    return out


# ---- what both evaluate_model_device routes share -------------------------------------------------
def model_path_t(model, times, delta_t, T):
    """The ``path_t`` the model's ``until_T`` call will return, before that call is made (the
    model's own schedule cache where it has one, so the walk is not made twice)."""
    from .schedule import Schedule
    cache = getattr(model, '_sched_cache', None)
    sched = cache.get(times, delta_t, T, True) if cache is not None else Schedule(times, delta_t, T, True)
    return sched.path_t


def need_cuda_device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('evaluate_model_device runs on the GPU only (device is {}); the host '
                         'route is evaluate_model'.format(dev))
    return dev


def as_f32(name, a, shape):
    """``a`` (numpy or CPU tensor) as a contiguous fp32 numpy array of ``shape``, or ValueError"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if tuple(a.shape) != tuple(shape):
        raise ValueError('{} must be {}, not {}'.format(name, list(shape), list(a.shape)))
    if a.dtype.kind not in 'fiub':
        raise ValueError('{} must be numeric, not {}'.format(name, a.dtype))
    return np.ascontiguousarray(a, dtype=np.float32)
