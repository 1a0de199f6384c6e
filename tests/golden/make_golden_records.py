"""
Generate tests/golden/g18_records_{physionet,climate}.npz by running the REFERENCE's two record
collates themselves.

Runs only in the build container (needs /root/reference; the reference never travels to the GPU
box).  The committed ``*.npz`` files hold data only: the raw records (``make_records`` /
``make_climate_records`` of njode_amd.synthetic_physionet, stored so that the fixtures do not
depend on the generator staying as it is), the batches' record indices and the reference's
outputs.  Usage:  python tests/golden/make_golden_records.py

* g18_records_physionet: ``variable_time_collate_fn1`` and ``normalize_masked_data``, executed
  from the reference's own source (latent_ODE/physionet_LODE.py cannot be imported here: it
  needs torchvision), in train and test layout, for two datasets (D = 5 and D = 41, 12 records,
  40 quantised times) and two batches each;
* g18_records_climate: ``GRU_ODE_Bayes.data_utils_gru_ode_bayes.custom_collate_fn`` on batches
  in the form ``ODE_Dataset.__getitem__`` builds (a frame indexed by ID with the columns Time,
  Value_*, Mask_*, fp32), two batches.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = '/root/reference'

from njode_amd import synthetic_physionet  # noqa: E402


def _functions(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(keep) == len(names), (path, names)
    exec(compile(ast.Module(keep, []), os.path.basename(path), 'exec'), ns)
    return [ns[n] for n in names]


def reference_physionet_collate():
    ns = {'torch': torch, 'np': np}
    (normalize,) = _functions(os.path.join(REF, 'latent_ODE', 'utils_LODE.py'),
                              ('normalize_masked_data',), ns)
    ns = {'torch': torch, 'np': np, 'utils': types.SimpleNamespace(normalize_masked_data=normalize)}
    (collate,) = _functions(os.path.join(REF, 'latent_ODE', 'physionet_LODE.py'),
                            ('variable_time_collate_fn1',), ns)
    return collate


def physionet():
    collate = reference_physionet_collate()
    args = types.SimpleNamespace(eval_input_prob=None, eval_input_seed=None)
    arrays = {}
    batches = {'a': [3, 0, 7, 1, 10, 5, 8], 'b': [11, 2, 2, 9, 4, 6]}
    for dim in (5, 41):
        records, data_min, data_max = synthetic_physionet.make_records(
            n_records=12, dim=dim, n_quant=40, n_obs_range=(3, 10), p_feature=0.3 if dim == 5 else 0.15,
            seed=18 + dim)
        data_max = data_max.copy()
        data_max[1] = 0.0             # an att_max of 0 is taken as 1
        p = 'd{}/'.format(dim)
        arrays[p + 'n_records'] = len(records)
        arrays[p + 'data_min'], arrays[p + 'data_max'] = data_min, data_max
        for n, (tt, vals, mask) in enumerate(records):
            arrays['{}rec{}/tt'.format(p, n)] = tt
            arrays['{}rec{}/vals'.format(p, n)] = vals
            arrays['{}rec{}/mask'.format(p, n)] = mask
        for name, idx in batches.items():
            arrays['{}{}/idx'.format(p, name)] = np.asarray(idx, dtype=np.int64)
            batch = [(str(n), torch.tensor(records[n][0]), torch.tensor(records[n][1]),
                      torch.tensor(records[n][2]), None) for n in idx]
            for layout in ('train', 'test'):
                # (normalize_masked_data writes into att_max: fresh tensors per call)
                res = collate(batch, args, data_type=layout, data_min=torch.tensor(data_min),
                              data_max=torch.tensor(data_max))
                q = '{}{}/{}/'.format(p, name, layout)
                assert res['times'].dtype == np.float32
                arrays[q + 'times'] = res['times']
                arrays[q + 'time_ptr'] = np.asarray(res['time_ptr'], dtype=np.int64)
                arrays[q + 'obs_idx'] = res['obs_idx'].numpy()
                arrays[q + 'X'] = res['X'].numpy().reshape(-1, dim)
                arrays[q + 'M'] = res['M'].numpy().reshape(-1, dim)
                if layout == 'test':
                    for k in ('times_val', 'vals_val', 'mask_val'):
                        arrays[q + k] = np.asarray(res[k])
                print('   physionet d={} batch {} {}: {} rows, {} times, {} empty slices'.format(
                    dim, name, layout, len(res['obs_idx']), len(res['times']),
                    int((np.diff(res['time_ptr']) == 0).sum())))
    np.savez_compressed(os.path.join(HERE, 'g18_records_physionet.npz'), **arrays)


def climate():
    import pandas as pd
    if not hasattr(np, 'int'):
        np.int = int            # the reference predates numpy 1.24
    sys.path.insert(0, REF)
    from GRU_ODE_Bayes.data_utils_gru_ode_bayes import custom_collate_fn
    dim = 5
    records = synthetic_physionet.make_climate_records(n_records=12, dim=dim, n_obs_range=(20, 40),
                                                      seed=18)
    arrays = {'n_records': len(records)}
    for n, (tt, vals, mask) in enumerate(records):
        arrays['rec{}/tt'.format(n)] = tt
        arrays['rec{}/vals'.format(n)] = vals
        arrays['rec{}/mask'.format(n)] = mask

    def item(n):
        tt, vals, mask = records[n]
        cols = {'Time': tt}
        cols.update({'Value_{}'.format(j): vals[:, j] for j in range(dim)})
        cols.update({'Mask_{}'.format(j): mask[:, j] for j in range(dim)})
        frame = pd.DataFrame(cols, index=pd.Index([n] * len(tt), name='ID')).astype(np.float32)
        return {'idx': n, 'y': np.zeros(1, dtype=np.float32), 'path': frame,
                'cov': np.zeros(1, dtype=np.float32), 'val_samples': None, 'store_last': False}

    # (a record may appear once here: the reference maps record IDs to batch positions)
    for name, idx in {'a': [3, 0, 7, 1, 10, 5, 8], 'b': [11, 2, 9, 4, 6]}.items():
        res = custom_collate_fn([item(n) for n in idx])
        q = name + '/'
        arrays[q + 'idx'] = np.asarray(idx, dtype=np.int64)
        arrays[q + 'times'] = np.asarray(res['times'])
        arrays[q + 'time_ptr'] = np.asarray(res['time_ptr'], dtype=np.int64)
        arrays[q + 'obs_idx'] = np.asarray(res['obs_idx'].numpy(), dtype=np.int64)
        arrays[q + 'X'] = res['X'].numpy()
        arrays[q + 'M'] = res['M'].numpy()
        print('   climate batch {}: {} rows, {} times ({})'.format(
            name, len(arrays[q + 'obs_idx']), len(arrays[q + 'times']), arrays[q + 'times'].dtype))
    np.savez_compressed(os.path.join(HERE, 'g18_records_climate.npz'), **arrays)


if __name__ == '__main__':
    physionet()
    climate()
