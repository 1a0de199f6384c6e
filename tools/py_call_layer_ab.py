"""A/B record of the Python call layer.  ``run OUT.json`` writes digests of what the autograd routes
and the three training loops compute, and the kernel launches of single steps; run it on two
trees with NJODE_LIB naming ONE library, then ``compare A B`` (two such files, or two
``bench.py --dump-outputs`` folders) prints every key and exits 1 unless all are equal."""
import copy, hashlib, json, os, sys, tempfile    # noqa: E401

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from njode_amd import _lib, data_utils, models, records, synthetic_physionet, train, train_records  # noqa: E402

NN = ((50, 'tanh'), (50, 'tanh'))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes())
    return h.hexdigest()[:16]


def dataset(n):
    hp = dict(copy.deepcopy(data_utils.hyperparam_default), nb_paths=n)
    out = data_utils.create_dataset('BlackScholes', hp, seed=0)
    return out[:3], out[3]


def model_and_batch(n=7, use_rnn=False, **options):
    (paths, obs, nb_obs), meta = dataset(n)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    args = (b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), meta['dt'],
            meta['maturity'], b['start_X'].cuda(), b['n_obs_ot'].cuda().int())
    torch.manual_seed(0)
    m = models.NJODE(1, 10, 1, NN, NN, NN, use_rnn, dropout_rate=0.1,
                     options=dict(options, device_outputs=True)).cuda().train()
    return m, args, dict(M=torch.ones_like(args[2])) if m.masked else {}


def autograd_routes(out):
    for name, kw in (('unmasked', {}), ('masked', dict(masked=True)), ('use_rnn', dict(use_rnn=True)),
                     ('library_op', dict(torch_library_op=True))):
        m, args, M = model_and_batch(**kw)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        for step in range(3):       # (deferred where plan_defer_ok allows it, else the helper stream)
            m.prefetch_plan(*args, **M)
            opt.zero_grad()
            hT, loss = m(*args, **M)
            (loss + (hT * hT).sum()).backward()
            opt.step()
            out['route/{}/{}'.format(name, step)] = sha(loss, hT, *[p.grad for p in m.parameters()],
                                                        *m.state_dict().values())


def loops(out):
    recs, mn, mx = synthetic_physionet.make_records(25, 41, n_quant=60, n_obs_range=(4, 12), seed=7)
    ids = np.array([0] + list(range(2, 25)))
    phys = records.RecordDataset.from_records(recs, mn, mx, device='cuda')
    clim = records.RecordDataset.from_records(
        synthetic_physionet.make_climate_records(40, 5, n_obs_range=(6, 14), seed=23), time_div=None,
        drop_unobserved=False, device='cuda')
    data, meta = dataset(300)
    runs = {'train': lambda **k: train.train(data, meta, batch_size=60, dropout_rate=0.1, **k),
            'records': lambda **k: train_records.train_records(
                phys, ids[:18], ids[18:], batch_size=8, hidden_size=41, dropout_rate=0.1, delta_t=1.0 / 60, **k),
            'climate': lambda **k: train_records.train_climate_records(
                clim, np.arange(24), np.arange(24, 32), np.arange(32, 40), batch_size=8, hidden_size=10,
                dropout_rate=0.1, delta_t=1.0, **k)}
    for name, run in runs.items():
        with tempfile.TemporaryDirectory() as tmp:
            kw = dict(log=lambda s: None, model_path=tmp, model_id=3, save_every=1)
            for tag, more in (('2ep', dict(epochs=2)), ('resumed', dict(epochs=3, resume_training=True))):
                m, met = run(**kw, **more)
                files = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)
                csv_rows = [r.split(',') for r in open(os.path.join(tmp, 'id-3', 'metric_id-3.csv')).read().split()]
                out['loop/{}/{}'.format(name, tag)] = [
                    sha(*m.state_dict().values()), [repr([r[0]] + r[3:]) for r in met],
                    [r[:2] + r[4:] for r in csv_rows], files]


def launches(out):
    def table(name, fn):
        _lib.profile_enable(1)
        _lib.profile_read()
        fn()
        out['launches/' + name] = {k: v[0] for k, v in sorted(_lib.profile_read().items())}
        _lib.profile_enable(0)
    m, args, _ = model_and_batch(100)
    opt = models.FusedAdam(m, lr=1e-3, weight_decay=0.0005)
    table('fused_step', lambda: (m.loss_and_grad(*args), opt.step()))
    table('autograd_step', lambda: m(*args)[1].backward())
    table('hT_backward', lambda: m(*args, get_loss=False)[0].sum().backward())
    for name, defer in (('deferred_prefetch', True), ('helper_stream_prefetch', False)):
        table(name, lambda: (m.prefetch_plan(*args, need_hT=False, defer=defer), m.loss_and_grad(*args)))


def compare(a, b):
    A, B = (({f: sha(np.load(os.path.join(d, f))) for f in os.listdir(d) if f.endswith('.npy')}
             if os.path.isdir(d) else json.load(open(d))) for d in (a, b))
    for k in sorted(set(A) | set(B)):
        print('{} {}: {}'.format('equal    ' if A.get(k) == B.get(k) else 'DIFFERENT', k, json.dumps(A.get(k))[:100]))
    return A == B


if __name__ == '__main__':
    if sys.argv[1] == 'compare':
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    out = {}
    for part in (autograd_routes, loops, launches):
        part(out)
        torch.cuda.synchronize()
    json.dump(out, open(sys.argv[2], 'w'), indent=1, sort_keys=True)
