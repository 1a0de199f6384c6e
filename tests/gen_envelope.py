"""The shape envelope of the shape-generic kernels, restated in Python from ``build_model`` /
``build_net`` (njode_amd/csrc/njode_gen.hip), together with the run-time branch labels of the
kernels (njode_gen.h) a model shape selects.  test_host_logic compares ``restate`` with
``njode_supported`` / ``njode_param_count``; test_hip_generic_envelope picks its GPU shapes by
the labels."""
from njode_amd import _lib

MAX_WIDTH = 1024            # NJODE_GEN_MAX_WIDTH
MAX_IN = MAX_WIDTH + 64     # widest layer input (build_net)
MAX_HIDDEN = _lib.MAX_HIDDEN
LDS_LIMIT = 160 * 1024
QU, RING, LCH = 4, 8, 4     # k-step padding, quads of a short row, quads per chunk of a long row
DW_TM = DW_TN = 4           # k_gen_dw: 16-unit tiles per block (outputs x inputs + bias)
XR = 4                      # observation values held in registers per thread (k_gen_fwd)

R_SIZES = 'sizes out of range'
R_MASKED = 'masked mode feeds the readout back'
R_RESIDUAL = 'residual:'
R_NHIDDEN = 'n_hidden out of range'
R_NET = 'network description out of range'
R_RNN = 'use_rnn: 4 x hidden_size'
R_LDS = 'exceed the 160 KB LDS'


def cdiv(a, b):
    return (a + b - 1) // b


def pad_to(v, m):
    return cdiv(v, m) * m


def dims_of(D, H, DO, nets, flags):
    """NjodeDims of a shape: ``nets`` is one (n_hidden, widths, acts) for all three networks
    (per_net = 0; widths / acts uniform) or three of them (ode, enc, readout; per_net = 1)."""
    if len(nets) == 3 and isinstance(nets[0], tuple):
        d = _lib.NjodeDims(D, H, DO, 0, 0, 0, flags)
        d.per_net = 1
        for i, (n, ws, acts) in enumerate(nets):
            d.nets[i].n_hidden = n
            for l in range(min(n, MAX_HIDDEN)):
                d.nets[i].width[l] = ws[l]
                d.nets[i].act[l] = acts[l]
        return d
    n, ws, acts = nets
    return _lib.NjodeDims(D, H, DO, n, ws[0] if n > 0 else 0, acts[0] if n > 0 else 0, flags)


def _layer(n_in, n_out, act, kind=0):
    Qp, QTp = pad_to(cdiv(n_in + 1, 4), QU), pad_to(cdiv(n_out, 4), QU)
    return dict(n_in=n_in, n_out=n_out, act=act, kind=kind, Qp=Qp, QTp=QTp, MT=cdiv(n_out, 16),
                MTT=cdiv(n_in, 16), P=n_in * n_out + n_out)


def restate(D, H, DO, nets, flags):
    """(None, model) if build_model accepts the shape, else (reason prefix, None).  ``model``: the
    layers (with the derived tables), P, img_rows, lds_bytes, nw, S."""
    masked, curt, res = flags & _lib.F_MASKED, flags & _lib.F_INPUT_CURRENT_T, flags & _lib.F_RESIDUAL
    rnn = flags & _lib.F_USE_RNN
    if D <= 0 or H <= 0 or DO <= 0 or D > 512 or H > 1024 or DO > 512:
        return R_SIZES, None
    if D != DO and masked:
        return R_MASKED, None
    enc_case = dec_case = 0
    if res:
        if D <= H:
            if H % D:
                return R_RESIDUAL, None
            enc_case = 1
        else:
            if D % H:
                return R_RESIDUAL, None
            enc_case = 2
        if H <= DO:
            if DO % H:
                return R_RESIDUAL, None
            dec_case = 1
        else:
            if H % DO:
                return R_RESIDUAL, None
            dec_case = 2
    per_net = len(nets) == 3 and isinstance(nets[0], tuple)
    if not per_net:
        if nets[0] < 0 or nets[0] > MAX_HIDDEN:
            return R_NHIDDEN, None
        nets = (nets, nets, nets)
    IN0 = D + H + (3 if curt else 2)
    layers, img_rows, max_mt, max_tb = [], 16, 1, 1
    for net, (n_in0, n_out0) in enumerate(((IN0, H), (2 * D if masked else D, H), (H, DO))):
        n, ws, acts = nets[net]
        if n < 0 or n > MAX_HIDDEN:
            return R_NET, None
        for l in range(n + 1):
            n_in = n_in0 if l == 0 else ws[l - 1]
            n_out = n_out0 if l == n else ws[l]
            if n_in <= 0 or n_out <= 0 or n_in > MAX_IN or n_out > MAX_WIDTH:
                return R_NET, None
            act = acts[l] if l < n else -1
            if l < n and act not in (_lib.ACT_TANH, _lib.ACT_RELU):
                return R_NET, None
            L = _layer(n_in, n_out, act)
            L['net'] = net
            layers.append(L)
            img_rows = max(img_rows, 4 * L['Qp'], 4 * L['QTp'], n_in + 1, n_out + 1)
            max_mt = max(max_mt, L['MT'], L['MTT'])
            max_tb = max(max_tb, cdiv(L['MT'], DW_TM) * cdiv(cdiv(n_in + 1, 16), DW_TN))
    P = sum(L['P'] for L in layers)
    if rnn:
        if 4 * H > MAX_WIDTH:
            return R_RNN, None
        L = _layer(D + H, 4 * H, -1, kind=1)
        L['net'] = 3
        L['P'] = 3 * H * D + 3 * H * H + 6 * H
        P += L['P']
        layers.append(L)
        img_rows = max(img_rows, 4 * L['Qp'], 4 * L['QTp'], L['n_out'] + 1)
        max_mt = max(max_mt, L['MT'])          # (not MTT: build_model leaves it out)
        max_tb = max(max_tb, cdiv(L['MT'], DW_TM) * cdiv(cdiv(L['n_in'] + 1, 16), DW_TN))
    img_rows = max(img_rows, IN0 + 4, 2 * D + 4, H + 4)
    img_rows = pad_to(img_rows + 4, 4)
    mx = max(D, DO)
    lds = (2 * img_rows * 16 + 2 * H * 16 + D * 16 + 5 * mx * 16 + 8 * 16 + 16) * 4
    if lds > LDS_LIMIT:
        return R_LDS, None
    return None, dict(layers=layers, P=P, img_rows=img_rows, lds_bytes=lds, max_mt=max_mt,
                      max_tb=max_tb, nw=min(max(max_mt, 4), 16), S=min(max(2048 // max_tb, 8), 256),
                      D=D, H=H, DO=DO, enc_case=enc_case, dec_case=dec_case, rnn=bool(rnn))


def _rows(Q):
    """Branch labels of layer_product over rows of Q quads."""
    if Q <= RING:
        return {'short'}
    nch = cdiv(Q, LCH)
    return {'long', 'long_odd' if nch % 2 else 'long_even', 'long_partial' if Q % LCH else 'long_full'}


def labels(model, nw=None):
    """The run-time branches this model takes at ``nw`` waves per workgroup (default: the model's)."""
    nw = nw or model['nw']
    out = set()
    for L in model['layers']:
        for Q, MT in ((L['Qp'] // QU, L['MT']), (L['QTp'] // QU, L['MTT'])):
            out |= _rows(Q)
            per = cdiv(MT, nw)
            if per > 1:
                out.add('tiles_per_wave_{}'.format(min(per, 4) if per <= 4 else '5+'))
            if cdiv(MT, per) < nw:
                out.add('idle_waves')
        tiles_n = cdiv(L['n_in'] + 1, 16)
        if L['n_in'] % 16 == 0:
            out.add('dw_bias_alone_in_tile')
        if tiles_n % DW_TN == 1:
            out.add('dw_bias_alone_in_block')
        if L['n_out'] % 16 or L['n_in'] % 16:
            out.add('dw_edge')
    last = model['layers'][-1]
    if last['QTp'] // QU > RING:    # the transposed table of the last layer reads into the padding
        out.add('prefetch_into_padding')
    out.add('S_{}'.format('256' if model['S'] == 256 else ('8' if model['S'] == 8 else 'mid')))
    out.add('x_regs' if model['D'] * 16 <= XR * 64 * nw else 'x_lds')
    if model['lds_bytes'] > 64 * 1024:
        out.add('lds_above_64k')
    if model['lds_bytes'] > LDS_LIMIT - 2048:
        out.add('lds_near_limit')
    if model['rnn']:
        out.add('gru')
    out.add('enc_case_{}'.format(model['enc_case']))
    out.add('dec_case_{}'.format(model['dec_case']))
    return out


def nets_of_cfg(cfg):
    """(nets argument of restate, flags) of a models.NJODE config dict."""
    from njode_amd import models
    o = cfg.get('options', {})
    flags = ((_lib.F_MASKED if o.get('masked') else 0) | (_lib.F_INPUT_CURRENT_T if o.get('input_current_t') else 0)
             | (_lib.F_RESIDUAL if o.get('residual_enc_dec', True) else 0)
             | (_lib.F_LOSS_EASY if o.get('which_loss') == 'easy' else 0)
             | (_lib.F_USE_RNN if cfg.get('use_rnn') else 0))
    descs = tuple(models._desc_of(cfg[k]) for k in ('ode_nn', 'enc_nn', 'readout_nn'))
    return descs, flags


def restate_cfg(cfg):
    nets, flags = nets_of_cfg(cfg)
    return restate(cfg['input_size'], cfg['hidden_size'], cfg['output_size'], nets, flags)
