"""The run-time choices of the float64 route, restated in Python from ``build_model`` / ``build_net`` /
``set_row_lanes`` / ``slab_count`` / ``make_layout`` of ``njode_amd/csrc/njode_f64.hip``: per layer the
lanes of the slab update, the workgroup size, the parameter count, the slab count of the adjoint sweep
and the workspace byte count, together with labels of the branches a call takes.  The case table of
``test_hip_f64_envelope`` is defined here too, so that ``test_f64_envelope_host`` can hold every case to
the library (``njode_f64_supported``, ``njode_f64_workspace_bytes``) without a GPU."""
import numpy as np

import gen_envelope
from njode_amd import _lib

MAX_WIDTH = gen_envelope.MAX_WIDTH          # NJODE_GEN_MAX_WIDTH
MAX_IN = gen_envelope.MAX_IN                # widest layer input (build_net)
MAX_HIDDEN = _lib.MAX_HIDDEN
LDS_LIMIT = 160 * 1024
MAX_SLABS = 2048
SLAB_BUDGET = 1 << 30
LOSS_THREADS = 256                          # tree_sum_256: one workgroup, striding over the paths
CLEAR_ELEMS = 2048 * 256                    # k_rows_clear: the grid's cap, striding beyond it

R_RNN = 'use_rnn: the GRU jump has no float64 kernels'
R_SIZES = 'sizes out of range'
R_MASKED = 'masked mode feeds the readout back'
R_RESIDUAL = 'residual:'
R_NHIDDEN = 'n_hidden out of range'
R_NET = 'network description out of range'
R_LDS = 'exceed the 160 KB LDS'


def _take(total, nbytes):
    """Arena::take: every array starts on a 256-byte boundary."""
    return total + ((nbytes + 255) & ~255)


def _residual(n_in, n_out):
    """(case, mult) of the FFNN residual from n_in to n_out, or None where the sizes do not divide."""
    if n_in <= n_out:
        return None if n_out % n_in else (1, n_out // n_in)
    return None if n_in % n_out else (2, n_in // n_out)


def restate(D, H, DO, nets, flags):
    """(None, model) if the float64 route takes the shape, else (reason prefix, None).  ``nets`` as
    ``gen_envelope.restate`` takes them.  ``model``: nets (three lists of layers, each a dict of n_in,
    n_out, act, w_off, b_off, cw, rows), nth, P, maxv, act_max, the residual cases and multipliers."""
    if flags & _lib.F_USE_RNN:
        return R_RNN, None
    if D <= 0 or H <= 0 or DO <= 0 or D > 512 or H > 1024 or DO > 512:
        return R_SIZES, None
    masked, curt = bool(flags & _lib.F_MASKED), bool(flags & _lib.F_INPUT_CURRENT_T)
    if masked and D != DO:
        return R_MASKED, None
    enc, dec = (0, 1), (0, 1)
    if flags & _lib.F_RESIDUAL:
        enc, dec = _residual(D, H), _residual(H, DO)
        if enc is None or dec is None:
            return R_RESIDUAL, None
    per_net = len(nets) == 3 and isinstance(nets[0], tuple)
    if not per_net:
        if nets[0] < 0 or nets[0] > MAX_HIDDEN:
            return R_NHIDDEN, None
        nets = (nets, nets, nets)
    IN0 = D + H + (3 if curt else 2)
    p_off, maxv, out, act_max = 0, 1, [], 0
    for (n, ws, acts), (n_in0, n_out0) in zip(nets, ((IN0, H), (2 * D if masked else D, H), (H, DO))):
        if n < 0 or n > MAX_HIDDEN:
            return R_NET, None
        layers, a_off = [], 0
        for l in range(n + 1):
            n_in = n_in0 if l == 0 else ws[l - 1]
            n_out = n_out0 if l == n else ws[l]
            if n_in <= 0 or n_out <= 0 or n_in > MAX_IN or n_out > MAX_WIDTH:
                return R_NET, None
            act = acts[l] if l < n else -1
            if l < n and act not in (_lib.ACT_TANH, _lib.ACT_RELU):
                return R_NET, None
            layers.append(dict(n_in=n_in, n_out=n_out, act=act, w_off=p_off, b_off=p_off + n_in * n_out, a_off=a_off))
            p_off += n_in * n_out + n_out
            a_off += n_in
            maxv = max(maxv, n_in, n_out)
        act_max = max(act_max, a_off)
        out.append(layers)
    nth = 64 if maxv <= 64 else (128 if maxv <= 128 else 256)
    for layers in out:
        for L in layers:       # set_row_lanes: the power of two that covers the row, capped at the workgroup
            lg = 0
            while (1 << lg) < L['n_in'] and (1 << lg) < nth:
                lg += 1
            L['cw'], L['rows'] = 1 << lg, nth >> lg
    lds = H + 3 * D + 2 * DO + H + max(H, DO) + act_max + 2 * H + D + 2 * DO + 2 * maxv   # lds_doubles(m, true)
    if lds * 8 > LDS_LIMIT:
        return R_LDS, None
    # (supported() asks the fp32 shape-generic family last: the envelope is its envelope minus use_rnn)
    why, _ = gen_envelope.restate(D, H, DO, nets, flags)
    if why is not None:
        return why, None
    return None, dict(nets=out, nth=nth, P=p_off, maxv=maxv, act_max=act_max, lds_bytes=lds * 8, D=D, H=H, DO=DO,
                      masked=masked, curt=curt, loss_easy=bool(flags & _lib.F_LOSS_EASY),
                      enc_case=enc[0], enc_mult=enc[1], dec_case=dec[0], dec_mult=dec[1],
                      depths=tuple(n for n, _, _ in nets))


def restate_cfg(cfg):
    nets, flags = gen_envelope.nets_of_cfg(cfg)
    return restate(cfg['input_size'], cfg['hidden_size'], cfg['output_size'], nets, flags)


def dims_of_cfg(cfg):
    nets, flags = gen_envelope.nets_of_cfg(cfg)
    return gen_envelope.dims_of(cfg['input_size'], cfg['hidden_size'], cfg['output_size'], nets, flags)


def layer_table(model):
    """[(n_in, n_out, cw, rows)] of every layer, in the flat vector's order."""
    return [(L['n_in'], L['n_out'], L['cw'], L['rows']) for layers in model['nets'] for L in layers]


def slab_count(model, B):
    return max(1, min(SLAB_BUDGET // (model['P'] * 8), MAX_SLABS, B))


def workspace_bytes(model, B, n_obs, n_times, K, flags):
    """make_layout(...).total"""
    no, k, t = max(n_obs, 1), max(K, 1), max(n_times, 1)
    H, D, P = model['H'], model['D'], model['P']
    total = 0
    for nbytes in (k * 8, k * 4, t * 4, t * 4, (t + 1) * 4, P * 8, t * B * 4, B * 8):
        total = _take(total, nbytes)
    if flags & _lib.C_SAVE_BWD:
        for nbytes in (k * B * H * 8, no * H * 8, no * D * 8, no * 4, B * D * 8, B * 4, slab_count(model, B) * P * 8):
            total = _take(total, nbytes)
    return total


VOCABULARY = {
    'nth_64', 'nth_128', 'nth_256', 'units_loop',
    'row_1_lane', 'row_idle_lanes', 'row_exact', 'row_strided', 'idle_row_groups',
    'depth_0', 'depth_0_all', 'depth_8', 'depth_mixed',
    'enc_case_0', 'enc_case_1_mult2+', 'enc_case_2_mult2+', 'dec_case_0', 'dec_case_1_mult2+', 'dec_case_2_mult2+',
    'masked', 'masked_enc_case_1_mult2+', 'masked_enc_case_2_mult2+', 'input_current_t', 'loss_easy', 'no_bias',
    'do_ne_d', 'S_eq_B', 'S_max_slabs', 'S_budget', 'S_uneven', 'loss_tree_strided', 'rows_clear_strided', 'no_rows', 'b1',
}


def labels(model, B, n_obs, n_times, K, bias=True):
    """The run-time branches a training call of ``model`` on such a batch takes.  Labels outside
    ``VOCABULARY`` (a residual case with trivial chunks) are reported as well."""
    out = {'nth_{}'.format(model['nth'])}
    nth = model['nth']
    for n_in, n_out, cw, rows in layer_table(model):
        if n_out > nth:
            out.add('units_loop')
        if n_in == 1:
            out.add('row_1_lane')
        elif n_in > nth:
            out.add('row_strided')
        elif n_in & (n_in - 1):
            out.add('row_idle_lanes')
        else:
            out.add('row_exact')
        if n_out < rows:
            out.add('idle_row_groups')
    depths = model['depths']
    if 0 in depths:
        out.add('depth_0')
    if not any(depths):
        out.add('depth_0_all')
    if MAX_HIDDEN in depths:
        out.add('depth_8')
    if {d % 2 for d in depths} == {0, 1}:
        out.add('depth_mixed')
    # a residual case counts as 'mult2+' only where its index arithmetic is not trivial: two chunks or
    # more of two units or more (D = 1 next to H = 10 is ten chunks of one unit: j % 1, i + c)
    for net, small in (('enc', min(model['D'], model['H'])), ('dec', min(model['H'], model['DO']))):
        case, mult = model[net + '_case'], model[net + '_mult']
        out.add('{}_case_{}'.format(net, case) if case == 0 else
                '{}_case_{}_{}'.format(net, case, 'mult2+' if mult >= 2 and small >= 2 else 'trivial'))
    for key in ('masked', 'loss_easy'):
        if model[key]:
            out.add(key)
    # (the adjoint of the encoder's residual reaches a parameter only through a masked model's Y_bj)
    for k in ('enc_case_1_mult2+', 'enc_case_2_mult2+'):
        if model['masked'] and k in out:
            out.add('masked_' + k)
    if model['curt']:
        out.add('input_current_t')
    if not bias:
        out.add('no_bias')
    if model['DO'] != model['D']:
        out.add('do_ne_d')
    S = slab_count(model, B)
    if S == B:
        out.add('S_eq_B')
    elif S == MAX_SLABS:
        out.add('S_max_slabs')
    else:
        assert S == SLAB_BUDGET // (model['P'] * 8) < B
        out.add('S_budget')
    if B % S:
        out.add('S_uneven')
    if B > LOSS_THREADS:
        out.add('loss_tree_strided')
    if n_times * B > CLEAR_ELEMS:
        out.add('rows_clear_strided')
    if n_obs == 0 and n_times == 0:
        out.add('no_rows')
    if B == 1:
        out.add('b1')
    return out


# ---- the case table of test_hip_f64_envelope ---------------------------------------------------------
REFUSED_ROWS = ('gru_h252', 'gru_masked_h252')      # use_rnn: outside this route's envelope
EDGES = (('b1', 'w128'), ('empty', 'w400'), ('longK', 'w64'))
BIG_B = 2100                                        # > MAX_SLABS, > LOSS_THREADS, no multiple of either
MASKED_BIG = ('masked_d20', 6)                      # (envelope row, n_grid) of the masked S_max_slabs case
CLEAR_K = 250                                       # 250 observation times x 2 100 paths = 525 000 > 524 288


def budget_cfg():
    """P = 7 373 333: 2^30 / 8P = 18 slabs."""
    wide = tuple((1024, 'tanh' if l % 2 else 'relu') for l in range(8))
    nn64 = ((64, 'tanh'),)
    return dict(input_size=1, hidden_size=10, output_size=1, ode_nn=wide, readout_nn=nn64, enc_nn=nn64,
                use_rnn=False, bias=True, dropout_rate=0.0, options={})


def deep8_cfg():
    """``deep_mixed`` of the envelope table with a live ODE network: its width-1 relu layer is dead at the
    table's weights, and with ``bias=False`` everything behind a dead layer is zero, so that row checks the
    ODE network's nine layers against gradients that are exactly zero.  Here: width 2 and tanh in its place."""
    ode = ((130, 'relu'), (17, 'tanh'), (64, 'relu'), (200, 'tanh'), (2, 'tanh'), (48, 'tanh'), (176, 'relu'),
           (33, 'tanh'))
    return dict(input_size=2, hidden_size=6, output_size=2, ode_nn=ode, enc_nn=None,
                readout_nn=((255, 'relu'), (17, 'tanh'), (128, 'relu')), use_rnn=False, bias=False, dropout_rate=0.0,
                options=dict(residual_enc_dec=False, input_current_t=True, which_loss='easy'))


def _deep8_batch():
    import hip_util
    b, dt, T = hip_util.exact_k_batch(17, 40, obs_per_path=4, seed=21, d=2)
    return b, dt, T, False


def masked_res_cfg(D, H):
    """A masked model whose encoder and readout residuals have two chunks of several units."""
    nn = ((24, 'tanh'), (24, 'relu'))
    return dict(input_size=D, hidden_size=H, output_size=D, ode_nn=nn, enc_nn=nn, readout_nn=nn, use_rnn=False,
                bias=True, dropout_rate=0.0, options=dict(masked=True, residual_enc_dec=True))


def _masked_small(D):
    from njode_amd import synthetic_physionet
    b = synthetic_physionet.make_batch(batch_size=9, dim=D, n_grid=20, n_obs_range=(2, 6), seed=30 + D)
    return b, b['delta_t'], b['T'], False


def _demo_big(K, obs):
    import hip_util
    b, dt, T = hip_util.exact_k_batch(BIG_B, K, obs_per_path=obs, seed=3)
    return b, dt, T, False


def _masked_big():
    from njode_amd import synthetic_physionet
    import test_hip_generic_envelope as env
    row, n_grid = MASKED_BIG
    b = synthetic_physionet.make_batch(batch_size=BIG_B, dim=env.ROWS[row][0]['input_size'], n_grid=n_grid,
                                       n_obs_range=(2, 5), seed=17)
    return b, b['delta_t'], b['T'], False


def _budget_batch():
    import hip_util
    b, dt, T = hip_util.exact_k_batch(20, 5, obs_per_path=2, seed=8)
    return b, dt, T, False


def _no_rows_batch():
    """Nobody is observed; four Euler steps up to T (an ``until_T`` call)."""
    import torch
    B = 6
    start = 1.0 + 0.1 * torch.arange(B, dtype=torch.float32).view(B, 1)
    b = dict(times=np.zeros(0), time_ptr=np.zeros(1, dtype=np.int64), X=torch.zeros(0, 1),
             obs_idx=torch.zeros(0, dtype=torch.long), start_X=start, n_obs_ot=torch.zeros(B, dtype=torch.long))
    return b, 0.25, 1.0, True


def case_table():
    """{name: (cfg, make)}; ``make()`` -> (batch, delta_t, T, until_T), deterministic."""
    import hip_util
    import test_hip_generic_envelope as env
    cases = {}
    for row, (cfg, _) in env.ROWS.items():
        if row not in REFUSED_ROWS:
            cases['env/' + row] = (cfg, lambda row=row: env.make_batch(row))
    for edge, row in EDGES:
        cases['env/{}/{}'.format(row, edge)] = (env.ROWS[row][0], lambda row=row, edge=edge: env.make_batch(row, edge))
    cases['deep8_live'] = (deep8_cfg(), _deep8_batch)
    cases['masked_res12'] = (masked_res_cfg(6, 12), lambda: _masked_small(6))
    cases['masked_res21'] = (masked_res_cfg(12, 6), lambda: _masked_small(12))
    cases['slab/demo_b2100'] =(hip_util.demo_cfg(), lambda: _demo_big(6, 2))
    cases['slab/masked_b2100'] = (env.ROWS[MASKED_BIG[0]][0], _masked_big)
    cases['slab/budget'] = (budget_cfg(), _budget_batch)
    cases['slab/rows_clear'] = (hip_util.demo_cfg(), lambda: _demo_big(CLEAR_K, 2))
    cases['no_rows'] = (hip_util.demo_cfg(), _no_rows_batch)
    return cases


def call_sizes(b, dt, T, until_T):
    """(B, n_obs, n_times, K) of the call ``NJODE64.forward`` makes of this batch."""
    from njode_amd.float64 import Schedule64
    s = Schedule64(b['times'], dt, T, until_T)
    return int(b['start_X'].shape[0]), int(b['time_ptr'][-1]), s.n_times, s.n_steps


def case_labels(cfg, sizes):
    why, model = restate_cfg(cfg)
    assert why is None, why
    return labels(model, *sizes, bias=cfg.get('bias', True))
