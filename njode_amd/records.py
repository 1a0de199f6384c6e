"""
Datasets of irregular, feature-masked records and their collate (C ABI: include/njode_records.h).

The masked NJ-ODE model of the PhysioNet and climate experiments is fed by two collates of the
reference: ``latent_ODE/physionet_LODE.py:428-544`` (``variable_time_collate_fn1``, train and
test layout, with ``utils_LODE.normalize_masked_data:370-385``) and
``GRU_ODE_Bayes/data_utils_gru_ode_bayes.py:235-303`` (``custom_collate_fn``).  Both take a
ragged list of records ``(tt [T_i], vals [T_i, D], mask [T_i, D])`` and return the batch's sorted
union of times with one row of ``X`` / ``M`` per (time, record) -- in Python loops over a dense
``[B, T, D]`` array, which takes seconds per batch at PhysioNet's sizes.

``RecordDataset`` holds the records once, as rows sorted by record then time whose times are
indices into the dataset's own sorted-unique time axis ``grid``.  A batch's time axis is a subset
of ``grid`` (``unique`` commutes with taking a subset, and the division by ``time_div`` is
elementwise), so a collate only ever orders and compares grid indices:

* ``collate_host``: the two reference collates restated in vectorised numpy on the store -- the
  repository's host route and the parity anchor of the kernels (needs no library);
* ``collate`` / ``prepare_batches`` + ``fill_batch``: the same batches, bit for bit, built by the
  HIP kernels from the copy of the store in HBM.  No CPU fallback: they call into
  ``libnjode_hip.so``;
* ``collate_val_host`` / ``collate_val`` / ``prepare_val_batches``: the climate validation layout
  (``ODE_Dataset(validation=True)``: observe up to ``T_val``, hold out each record's next
  ``max_val_samples`` rows), in the same two routes.  It has methods of its own: ``LAYOUTS`` are
  the two layouts of ``collate``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr_arg as _ptr, stream_arg as _stream
from .device_data import _host_rows

LAYOUTS = ('train', 'test')


def _as_numpy(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class RecordDataset:
    """Record store: ``grid`` float64 ``[G]`` (host), ``row_ptr`` int32 ``[N + 1]``, ``row_g`` int32
    ``[R]``, ``vals`` fp32 ``[R, D]``, ``mask`` u8 ``[R, D]``, ``att_min`` / ``att_max`` fp32
    ``[D]`` or None -- numpy arrays on the host and, with a ``device``, tensors in HBM."""

    def __init__(self, grid, row_ptr, row_g, vals, mask, att_min, att_max, drop_unobserved,
                 device=None):
        self.grid = np.ascontiguousarray(grid, dtype=np.float64)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.row_g = np.ascontiguousarray(row_g, dtype=np.int32)
        self.vals = np.ascontiguousarray(vals, dtype=np.float32)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self.att_min = None if att_min is None else np.ascontiguousarray(att_min, dtype=np.float32)
        self.att_max = None if att_max is None else np.ascontiguousarray(att_max, dtype=np.float32)
        self.drop_unobserved = bool(drop_unobserved)
        self.n_records = len(self.row_ptr) - 1
        self.n_rows, self.dim = self.vals.shape
        self.n_grid = len(self.grid)
        self.device = None if device is None else torch.device(device)
        self._dev = None
        if self.device is not None:
            up = lambda a: None if a is None else torch.from_numpy(a).to(self.device)  # noqa: E731
            self._dev = {k: up(getattr(self, k)) for k in
                         ('row_ptr', 'row_g', 'vals', 'mask', 'att_min', 'att_max')}
            d = self._dev
            self._store = _lib.NjodeRecordStore(
                self.n_records, self.n_rows, self.dim, self.n_grid, int(self.drop_unobserved), 0,
                d['row_ptr'].data_ptr(), d['row_g'].data_ptr(), d['vals'].data_ptr(),
                d['mask'].data_ptr(),
                d['att_min'].data_ptr() if d['att_min'] is not None else None,
                d['att_max'].data_ptr() if d['att_max'] is not None else None)

    def __len__(self):
        return self.n_records

    # -- construction --------------------------------------------------------------------
    @classmethod
    def from_records(cls, records, data_min=None, data_max=None, time_div=48.0,
                     drop_unobserved=True, device='cuda'):
        """``records``: a list of ``(tt [T_i], vals [T_i, D], mask [T_i, D])`` numpy arrays / CPU
        tensors, ``tt`` fp32 and strictly increasing, one ``D`` for all, ``mask`` entries 0 or 1.
        ``data_min`` / ``data_max`` ``[D]``: the ``att_min`` / ``att_max`` of
        ``normalize_masked_data`` (both or neither).  ``grid`` is ``np.unique`` of all fp32 ``tt``,
        divided by ``np.float32(time_div)`` in fp32 (``combined_tt / 48.``; None: no division) and
        widened to float64.  ``device=None`` keeps the store on the host only.  ``ValueError``
        for anything else."""
        if len(records) == 0:
            raise ValueError('no records')
        if (data_min is None) != (data_max is None):
            raise ValueError('data_min and data_max come together or not at all')
        tts, vs, ms = [], [], []
        dim = None
        for i, (tt, vals, mask) in enumerate(records):
            tt, vals, mask = _as_numpy(tt), _as_numpy(vals), _as_numpy(mask)
            if tt.ndim != 1 or vals.ndim != 2 or mask.shape != vals.shape or len(tt) != len(vals):
                raise ValueError('record {}: tt [T], vals [T, D] and mask [T, D] expected'.format(i))
            if dim is None:
                dim = vals.shape[1]
            if vals.shape[1] != dim or dim == 0:
                raise ValueError('record {} has {} features, the first has {}'.format(
                    i, vals.shape[1], dim))
            tt = tt.astype(np.float32)
            if not np.all(np.isfinite(tt)) or np.any(np.diff(tt) <= 0):
                raise ValueError('record {}: tt must be finite and strictly increasing'.format(i))
            if np.any((mask != 0) & (mask != 1)):
                raise ValueError('record {}: mask entries must be 0 or 1'.format(i))
            tts.append(tt)
            vs.append(vals.astype(np.float32))
            ms.append(mask.astype(np.uint8))
        all_tt = np.concatenate(tts)
        if len(all_tt) == 0:
            raise ValueError('the records have no rows')
        uniq, row_g = np.unique(all_tt, return_inverse=True)
        if time_div is not None:
            uniq = uniq / np.float32(time_div)        # fp32 / fp32, as torch's combined_tt / 48.
        row_ptr = np.concatenate([[0], np.cumsum([len(t) for t in tts])])
        if row_ptr[-1] >= 2 ** 31:
            raise ValueError('more rows than an int32 index holds')
        att = []
        for a in (data_min, data_max):
            if a is not None:
                a = _as_numpy(a).astype(np.float32).reshape(-1)
                if len(a) != dim:
                    raise ValueError('data_min / data_max must have one entry per feature')
            att.append(a)
        return cls(uniq.astype(np.float64), row_ptr, row_g.reshape(-1), np.concatenate(vs),
                   np.concatenate(ms), att[0], att[1], drop_unobserved, device)

    # -- the host route ------------------------------------------------------------------
    def _normalise(self, vals, mask):
        """``normalize_masked_data``: ``(data - att_min) / att_max`` in fp32 with an ``att_max`` of 0
        taken as 1 -- it divides by ``att_max``, not by the range -- and 0 where the mask is 0;
        without normalisation the raw values."""
        if self.att_min is None:
            return vals
        att_max = np.where(self.att_max == 0, np.float32(1), self.att_max)
        x = (vals - self.att_min[None, :]) / att_max[None, :]
        x[mask == 0] = 0
        return x.astype(np.float32)

    def _batch_rows(self, idx):
        """Rows of the batch: (batch position, grid index, row) of every row, by batch position."""
        idx = _host_rows(idx, self.n_records).astype(np.int64)
        if len(idx) == 0:
            raise ValueError('empty batch')
        lo, n = self.row_ptr[idx].astype(np.int64), np.diff(self.row_ptr)[idx].astype(np.int64)
        rb = np.repeat(np.arange(len(idx)), n)
        rid = np.repeat(lo - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(n.sum())
        return len(idx), rb, self.row_g[rid].astype(np.int64), rid

    def _split(self, present_g, layout):
        """``(g_hi, held-out grid indices)``: the train layout collates every time; the test layout
        the first ``len(times) // 2`` of the batch's own union (``physionet_LODE.py:489-496``)."""
        if layout not in LAYOUTS:
            raise ValueError("layout must be 'train' or 'test'")
        if layout == 'train' or len(present_g) == 0:
            return self.n_grid, present_g[:0]
        n_t = len(present_g) // 2
        return int(present_g[n_t]), present_g[n_t:]

    def collate_host(self, idx, layout='train'):
        """The batch the reference's collate builds for records ``idx`` (batch order), on the host:
        ``times`` float64, ``time_ptr`` int64, ``X`` / ``M`` fp32 CPU tensors with rows sorted by time
        then batch position, ``obs_idx`` / ``n_obs_ot`` int64 tensors, ``start_X = zeros [B, D]``,
        ``batch_size``; in test layout also ``times_val`` float64 and ``vals_val`` / ``mask_val`` fp32
        numpy ``[B, n_val, D]``.  ``eval_input_prob`` is not offered."""
        B, rb, rg, rid = self._batch_rows(idx)
        present_g = np.unique(rg)
        g_hi, val_g = self._split(present_g, layout)
        mask = self.mask[rid]
        kept = mask.any(axis=1) if self.drop_unobserved else np.ones(len(rid), dtype=bool)
        sel = np.nonzero(kept & (rg < g_hi))[0]
        sel = sel[np.lexsort((rb[sel], rg[sel]))]                # by time, then batch position
        obs_g = present_g[present_g < g_hi]
        count = np.bincount(rg[sel], minlength=self.n_grid)
        out = {
            'times': self.grid[obs_g].copy(),
            'time_ptr': np.concatenate([[0], np.cumsum(count[obs_g])]).astype(np.int64),
            'X': torch.from_numpy(self._normalise(self.vals[rid[sel]], mask[sel])),
            'M': torch.from_numpy(mask[sel].astype(np.float32)),
            'obs_idx': torch.from_numpy(rb[sel].astype(np.int64)),
            'n_obs_ot': torch.from_numpy(np.bincount(rb[sel], minlength=B).astype(np.int64)),
            'start_X': torch.zeros(B, self.dim),
            'batch_size': B,
        }
        if layout == 'test':
            late = np.nonzero(rg >= g_hi)[0]
            v = np.searchsorted(val_g, rg[late])
            vals_val = np.zeros((B, len(val_g), self.dim), dtype=np.float32)
            mask_val = np.zeros((B, len(val_g), self.dim), dtype=np.float32)
            vals_val[rb[late], v] = self._normalise(self.vals[rid[late]], mask[late])
            mask_val[rb[late], v] = mask[late]
            out.update(times_val=self.grid[val_g].copy(), vals_val=vals_val, mask_val=mask_val)
        return out

    # -- the climate validation layout, host route -----------------------------------------
    def val_cut(self, T_val):
        """``g_cut``: the number of grid points ``<= float32(T_val)`` -- the reference compares its
        fp32 ``Time`` column with ``T_val``.  A row is observed if ``row_g < g_cut`` and held out
        otherwise; 0 leaves nothing observed, ``n_grid`` nothing held out."""
        if not np.isfinite(T_val):
            raise ValueError('T_val must be finite, not {}'.format(T_val))
        return int(np.searchsorted(self.grid, np.float64(np.float32(T_val)), side='right'))

    def eligible(self, idx, T_val=150):
        """The records of ``idx``, in their order, that a validation or test set keeps
        (``ODE_Dataset.__init__:112-123``): at least one row ``<= T_val`` and one ``> T_val``."""
        idx = _host_rows(idx, self.n_records).astype(np.int64)
        g_cut = self.val_cut(T_val)
        lo, hi = self.row_ptr[idx].astype(np.int64), self.row_ptr[idx + 1].astype(np.int64)
        some = hi > lo
        first = self.row_g[np.where(some, lo, 0)]
        last = self.row_g[np.where(some, hi - 1, 0)]
        return idx[some & (first < g_cut) & (last >= g_cut)]

    def _check_val(self, T_val, max_val_samples):
        if self.drop_unobserved:
            raise ValueError('the validation layout belongs to the collate that keeps every row: '
                             'a store with drop_unobserved=False')
        if int(max_val_samples) != max_val_samples or max_val_samples < 1:
            raise ValueError('max_val_samples must be a positive integer')
        return self.val_cut(T_val), int(max_val_samples)

    def _host_val_idx(self, idx):
        idx = _host_rows(idx, self.n_records)
        if len(idx) == 0:
            raise ValueError('empty batch')
        if len(np.unique(idx)) != len(idx):
            raise ValueError('a record appears twice in the batch: the validation layout maps '
                             'records to batch positions')
        return idx

    def collate_val_host(self, idx, T_val=150, max_val_samples=3):
        """The batch ``ODE_Dataset(validation=True, val_options={'T_val', 'max_val_samples'})`` +
        ``custom_collate_fn`` build for records ``idx`` (batch order), on the host
        (``data_utils_gru_ode_bayes.py:160-183, 257-265``).  The keys of ``collate_host``'s train
        layout for the rows with time ``<= T_val``, and for the first ``max_val_samples`` later
        rows of every record, sorted by (record, time): ``X_val`` / ``M_val`` fp32 CPU tensors
        ``[L, D]``, ``times_val`` float64 ``[L]``, ``index_val`` int64 ``[L]`` (batch position of the
        row's record); ``pat_idx`` the records.  ``climate_eval.evaluate_model`` takes the dict as
        it is.  An empty observed part has zero rows and ``time_ptr = [0]``."""
        g_cut, max_val = self._check_val(T_val, max_val_samples)
        idx = self._host_val_idx(idx).astype(np.int64)
        B, rb, rg, rid = self._batch_rows(idx)
        mask = self.mask[rid]
        # observed part: the climate collate restricted to g < g_cut (by time, then batch position)
        sel = np.nonzero(rg < g_cut)[0]
        sel = sel[np.lexsort((rb[sel], rg[sel]))]
        obs_g = np.unique(rg[sel])
        count = np.bincount(rg[sel], minlength=self.n_grid)
        # held-out part: rank of a row among its record's rows after the cut
        late = rg >= g_cut
        n_rows = np.bincount(rb, minlength=B)
        start = np.concatenate([[0], np.cumsum(n_rows)[:-1]])
        rank = np.arange(len(rb)) - start[rb] - np.bincount(rb[~late], minlength=B)[rb]
        val = np.nonzero(late & (rank < max_val))[0]
        val = val[np.lexsort((rg[val], rb[val], idx[rb[val]]))]   # by record, (position,) time
        return {
            'times': self.grid[obs_g].copy(),
            'time_ptr': np.concatenate([[0], np.cumsum(count[obs_g])]).astype(np.int64),
            'X': torch.from_numpy(self._normalise(self.vals[rid[sel]], mask[sel])),
            'M': torch.from_numpy(mask[sel].astype(np.float32)),
            'obs_idx': torch.from_numpy(rb[sel].astype(np.int64)),
            'n_obs_ot': torch.from_numpy(np.bincount(rb[sel], minlength=B).astype(np.int64)),
            'start_X': torch.zeros(B, self.dim),
            'batch_size': B,
            'pat_idx': idx.tolist(),
            'X_val': torch.from_numpy(self._normalise(self.vals[rid[val]], mask[val])),
            'M_val': torch.from_numpy(mask[val].astype(np.float32)),
            'times_val': self.grid[rg[val]].copy(),
            'index_val': rb[val].astype(np.int64),
        }

    # -- the device route ----------------------------------------------------------------
    def _need_device(self):
        if self._dev is None:
            raise RuntimeError('this RecordDataset was built with device=None: only collate_host')

    def _ws(self, B):
        need = C.c_size_t(0)
        _lib.check(_lib.lib().njode_records_bytes(self.n_grid, B, C.byref(need)))
        return torch.empty(need.value, dtype=torch.uint8, device=self.device)

    def prepare_batches(self, idx_list, layout='train'):
        """Phase 1 of the collate for MANY batches (an epoch) at once: ONE upload of the indices,
        the count kernels of all batches enqueued back to back, ONE copy back, ONE wait.
        ``idx_list``: records of each batch (array-likes on the host, batch order); ``ValueError``
        for a record outside ``[0, n_records)``, before anything is uploaded or launched.  Returns
        one descriptor per batch for ``fill_batch``.  The descriptors of one call share one
        workspace (sized for the largest batch): fill them on one stream, in any order."""
        self._need_device()
        if layout not in LAYOUTS:
            raise ValueError("layout must be 'train' or 'test'")
        sizes = [len(ix) for ix in idx_list]
        if not sizes or min(sizes) <= 0:
            raise ValueError('empty batch')
        flat = _host_rows(np.concatenate([np.asarray(ix).reshape(-1) for ix in idx_list]),
                          self.n_records)
        idx_dev = torch.as_tensor(flat).to(self.device)
        return self._prepare(idx_dev, sizes, layout)

    def _prepare(self, idx_dev, sizes, layout):
        L = _lib.lib()
        dev = self.device
        n, G = len(sizes), self.n_grid
        flags = torch.empty((n, 2, G), dtype=torch.int32, device=dev)     # [present | count]
        ws = self._ws(max(sizes))
        offs = np.concatenate([[0], np.cumsum(sizes)])
        with torch.cuda.device(dev):
            st = _stream(dev)
            for i in range(n):
                lo = int(offs[i])
                _lib.check(L.njode_records_count(
                    C.byref(self._store), C.c_void_p(idx_dev.data_ptr() + 4 * lo), sizes[i],
                    _ptr(flags[i, 0]), _ptr(flags[i, 1]), _ptr(ws), ws.numel(), st))
            flags_host = flags.cpu().numpy()                              # one copy, one wait
        out = []
        for i in range(n):
            lo, hi = int(offs[i]), int(offs[i + 1])
            present_g = np.nonzero(flags_host[i, 0])[0]
            g_hi, val_g = self._split(present_g, layout)
            obs_g = present_g[present_g < g_hi]
            time_ptr = np.concatenate([[0], np.cumsum(flags_host[i, 1][obs_g])]).astype(np.int64)
            out.append({'times': self.grid[obs_g].copy(), 'time_ptr': time_ptr,
                        'idx': idx_dev[lo:hi], 'B': hi - lo, 'flags': flags[i], 'g_hi': g_hi,
                        'layout': layout, 'times_val': self.grid[val_g].copy(), 'ws': ws})
        return out

    def fill_batch(self, prep):
        """Phase 2 (and, in test layout, 2b) for one descriptor of ``prepare_batches``: kernel
        launches only, no host wait.  Same batch, bit for bit, as ``collate`` builds.  A descriptor
        of ``prepare_val_batches`` gives the batch ``collate_val`` builds."""
        self._need_device()
        L = _lib.lib()
        dev = self.device
        B, D = prep['B'], self.dim
        n_obs = int(prep['time_ptr'][-1])
        f32, i32 = torch.float32, torch.int32
        X = torch.empty((n_obs, D), dtype=f32, device=dev)
        M = torch.empty((n_obs, D), dtype=f32, device=dev)
        obs_idx = torch.empty(n_obs, dtype=i32, device=dev)
        n_obs_ot = torch.empty(B, dtype=i32, device=dev)
        ws, flags = prep['ws'], prep['flags']
        null = C.c_void_p(0)
        out = {'times': prep['times'], 'time_ptr': prep['time_ptr'], 'X': X, 'M': M,
               'obs_idx': obs_idx, 'n_obs_ot': n_obs_ot,
               'start_X': torch.zeros((B, D), dtype=f32, device=dev), 'batch_size': B}
        with torch.cuda.device(dev):
            st = _stream(dev)
            _lib.check(L.njode_records_fill(
                C.byref(self._store), _ptr(prep['idx']), B, _ptr(flags[1]), 0, prep['g_hi'], n_obs,
                _ptr(X) if n_obs else null, _ptr(M) if n_obs else null,
                _ptr(obs_idx) if n_obs else null, _ptr(n_obs_ot), _ptr(ws), ws.numel(), st))
            if prep['layout'] == 'test':
                n_val = len(prep['times_val'])
                vals_val = torch.empty((B, n_val, D), dtype=f32, device=dev)
                mask_val = torch.empty((B, n_val, D), dtype=f32, device=dev)
                _lib.check(L.njode_records_heldout(
                    C.byref(self._store), _ptr(prep['idx']), B, _ptr(flags[0]), prep['g_hi'], n_val,
                    _ptr(vals_val) if n_val else null, _ptr(mask_val) if n_val else null,
                    _ptr(ws), ws.numel(), st))
                out.update(times_val=prep['times_val'], vals_val=vals_val, mask_val=mask_val)
            if prep['layout'] == 'validation':
                n_val = prep['L']
                X_val = torch.empty((n_val, D), dtype=f32, device=dev)
                M_val = torch.empty((n_val, D), dtype=f32, device=dev)
                g_val = torch.empty(n_val, dtype=i32, device=dev)
                index_val = torch.empty(n_val, dtype=i32, device=dev)
                ws_val = prep['ws_val']
                _lib.check(L.njode_records_val_fill(
                    C.byref(self._store), _ptr(prep['idx']), B, prep['g_hi'], prep['max_val'],
                    _ptr(prep['val_ptr']), n_val, _ptr(X_val) if n_val else null,
                    _ptr(M_val) if n_val else null, _ptr(g_val) if n_val else null,
                    _ptr(index_val) if n_val else null, _ptr(ws_val), ws_val.numel(), st))
                out.update(X_val=X_val, M_val=M_val, index_val=index_val,
                           times_val=self._grid_device()[g_val.long()], pat_idx=prep['pat_idx'])
        return out

    def _grid_device(self):
        if self._dev.get('grid') is None:
            self._dev['grid'] = torch.from_numpy(self.grid).to(self.device)
        return self._dev['grid']

    def _prepare_val(self, idx_dev, sizes, pat_idx, g_cut, max_val):
        L = _lib.lib()
        dev = self.device
        n, G = len(sizes), self.n_grid
        offs = np.concatenate([[0], np.cumsum(sizes)])
        # per batch [present G | count G | val_ptr B + 1], all batches in one buffer: one copy back
        seg = np.concatenate([[0], np.cumsum([2 * G + B + 1 for B in sizes])])
        buf = torch.empty(int(seg[-1]), dtype=torch.int32, device=dev)
        ws = self._ws(max(sizes))
        need = C.c_size_t(0)
        _lib.check(L.njode_records_val_bytes(max(sizes), C.byref(need)))
        ws_val = torch.empty(need.value, dtype=torch.uint8, device=dev)
        parts = []
        with torch.cuda.device(dev):
            st = _stream(dev)
            for i in range(n):
                lo, s0, B = int(offs[i]), int(seg[i]), sizes[i]
                flags = buf[s0:s0 + 2 * G].view(2, G)
                val_ptr = buf[s0 + 2 * G:s0 + 2 * G + B + 1]
                idx_i = C.c_void_p(idx_dev.data_ptr() + 4 * lo)
                _lib.check(L.njode_records_count(
                    C.byref(self._store), idx_i, B, _ptr(flags[0]), _ptr(flags[1]), _ptr(ws),
                    ws.numel(), st))
                _lib.check(L.njode_records_val_count(
                    C.byref(self._store), idx_i, B, g_cut, max_val, _ptr(val_ptr), _ptr(ws_val),
                    ws_val.numel(), st))
                parts.append((flags, val_ptr))
            host = buf.cpu().numpy()                                      # one copy, one wait
        out = []
        for i in range(n):
            lo, hi, s0, B = int(offs[i]), int(offs[i + 1]), int(seg[i]), sizes[i]
            present, count = host[s0:s0 + G], host[s0 + G:s0 + 2 * G]
            obs_g = np.nonzero(present[:g_cut])[0]
            time_ptr = np.concatenate([[0], np.cumsum(count[obs_g])]).astype(np.int64)
            out.append({'times': self.grid[obs_g].copy(), 'time_ptr': time_ptr,
                        'idx': idx_dev[lo:hi], 'B': B, 'flags': parts[i][0], 'g_hi': g_cut,
                        'layout': 'validation', 'ws': ws, 'ws_val': ws_val,
                        'val_ptr': parts[i][1], 'L': int(host[s0 + 2 * G + B]),
                        'max_val': max_val, 'pat_idx': pat_idx[i]})
        return out

    def prepare_val_batches(self, idx_list, T_val=150, max_val_samples=3):
        """``prepare_batches`` for the climate validation layout: ONE upload of the indices, the
        count kernels of the observed and of the held-out part of all batches enqueued back to
        back, ONE copy back (per-time counts and the number of held-out rows ``L`` of every batch),
        ONE wait.  Returns one descriptor per batch for ``fill_batch``.  ``ValueError``, before
        anything is uploaded or launched: a record outside the store or twice in a batch, an empty
        batch, ``max_val_samples < 1``, a non-finite ``T_val``, a store with
        ``drop_unobserved=True``."""
        self._need_device()
        g_cut, max_val = self._check_val(T_val, max_val_samples)
        lists = [self._host_val_idx(ix) for ix in idx_list]
        if not lists:
            raise ValueError('empty batch')
        idx_dev = torch.from_numpy(np.concatenate(lists)).to(self.device)
        return self._prepare_val(idx_dev, [len(ix) for ix in lists], [ix.tolist() for ix in lists],
                                 g_cut, max_val)

    def collate_val(self, idx, T_val=150, max_val_samples=3):
        """``collate_val_host`` on the GPU: ``X``, ``M``, ``obs_idx`` (int32), ``n_obs_ot`` (int32),
        ``start_X``, ``X_val``, ``M_val``, ``index_val`` (int32) and ``times_val`` (float64, the
        device copy of ``grid`` gathered at the rows' grid indices) are device tensors; ``times`` and
        ``time_ptr`` numpy arrays.  One host wait, like ``collate``.

        Records given on the host are checked like ``prepare_val_batches`` checks them.  A device
        tensor is used as it is, unchecked: an entry outside the store counts as a record without
        rows, and of a record that appears twice the held-out rows are listed by batch position."""
        self._need_device()
        g_cut, max_val = self._check_val(T_val, max_val_samples)
        if torch.is_tensor(idx) and idx.device.type != 'cpu':
            idx_dev = idx.to(self.device).to(torch.int32).contiguous().reshape(-1)
            if idx_dev.numel() == 0:
                raise ValueError('empty batch')
            pat_idx = idx_dev
        else:
            host = self._host_val_idx(idx)
            idx_dev, pat_idx = torch.from_numpy(host).to(self.device), host.tolist()
        return self.fill_batch(
            self._prepare_val(idx_dev, [idx_dev.numel()], [pat_idx], g_cut, max_val)[0])

    def collate(self, idx, layout='train'):
        """``collate_host`` on the GPU: ``X``, ``M``, ``obs_idx`` (int32), ``n_obs_ot`` (int32),
        ``start_X`` and, in test layout, ``vals_val`` / ``mask_val`` are device tensors; ``times``,
        ``time_ptr`` and ``times_val`` numpy arrays.  The per-time counts must reach the host before
        ``X`` can be sized, so the call waits once for its own first kernels
        (``prepare_batches`` + ``fill_batch`` is the form with one wait per epoch).

        Records given on the host are checked (``ValueError`` outside ``[0, n_records)``).  A
        device tensor is used as it is, unchecked -- a check would cost a host wait per batch:
        its entries are the caller's responsibility."""
        self._need_device()
        if layout not in LAYOUTS:
            raise ValueError("layout must be 'train' or 'test'")
        if torch.is_tensor(idx) and idx.device.type != 'cpu':
            idx_dev = idx.to(self.device).to(torch.int32).contiguous().reshape(-1)
        else:
            idx_dev = torch.from_numpy(_host_rows(idx, self.n_records)).to(self.device)
        if idx_dev.numel() == 0:
            raise ValueError('empty batch')
        return self.fill_batch(self._prepare(idx_dev, [idx_dev.numel()], layout)[0])
