"""The kernel route of a call, pinned without a GPU.

``njode_route.h`` is host code: ``size_call`` decides what a call's workspace is sized for, ``route_call``
which kernels its launchers (``njode_cfg.hip``) run.  ``tools/route_table.cpp`` prints both for a grid of
calls -- both sides of every threshold, the wrapper's flag sets, tail / dropout / hT -- for every distinct
capability row of ``njode_amd.build.CONFIGS`` (from ``caps()``, the one Python restatement of the kernels'
capability predicates).  The switches are read once per process, so the program runs once per switch set;
its output must equal ``tests/golden/route_table.txt`` -- the default set's table in full, every other set
as the cells in which it differs from the default, ``<lines>: <column>=<value> ...`` (regenerate with
``python -c "import test_route_table as t; t.write_golden()"`` from this directory, and read the diff).

Besides the table, every line is checked against the route's invariants: the dispatch part is admitted by
the sizing part, block counts fit their slabs, a saving forward and its backward run the same kernel
family, and each launch-level field equals the expression the launchers evaluated themselves before the
route carried it (restated once, in ``launcher_expressions``)."""
import os
import shutil
import subprocess

import pytest

from njode_amd.build import CONFIGS, _hipcc
from test_hip_route_matrix import ENVS, caps

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, 'golden', 'route_table.txt')

SWITCH_SETS = {
    'default': {},
    'tiles': ENVS['tiles'],
    'mfma1': ENVS['mfma1'],
    'ode_valu': {'NJODE_ODE': 'valu'},
    'lock4_0': {'NJODE_LOCK4': '0'},
    'drop_bits_ahead_0': {'NJODE_DROP_BITS_AHEAD': '0'},
    'chain_wpb_2': {'NJODE_CHAIN_WPB': '2'},
}
CAP_ORDER = ('HAS_MFMA', 'HAS_SPLIT', 'HAS_MFMA_LOCK', 'HAS_MFMA_SWEEP', 'HAS_Q4', 'HAS_CHAIN', 'HAS_SEG_CHAIN')
ODE_MFMA, ODE_VALU = 0, 1
VALU, WAVE1, TILE4, CHAIN = 0, 1, 2, 3          # LockKind
C_TRAIN, C_RETURN_PATH, C_SAVE = 0x1, 0x4, 0x8
CHAIN_MAX_WAVES = 8


def cap_rows():
    """(hidden_size, width, masked | use_rnn flags, capability bits) of the compiled shapes, one per distinct
    value of what the route reads of a shape: hidden_size <= 16, width < 64, the flags and the bits."""
    rows = {}
    for c in CONFIGS:
        d, H, DO, nh, W, act, masked, curt, res, rnn = c
        k = caps(c)
        W = W if nh else 0
        row = (H, W, masked * 0x1 + rnn * 0x10) + tuple(int(k[n]) for n in CAP_ORDER)
        rows.setdefault((H <= 16, W < 64) + row[2:], row)
    return list(rows.values())


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cc = _hipcc()
    if not (os.path.exists(cc) or shutil.which(cc)):
        pytest.skip('no hipcc')
    exe = str(tmp_path_factory.mktemp('route_table') / 'route_table')
    p = subprocess.run([cc, '--cuda-host-only', '-std=c++17', '-O0', os.path.join(REPO, 'tools', 'route_table.cpp'),
                        '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return exe


def run_table(exe, switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith('NJODE_')}
    stdin = ''.join(' '.join(map(str, r)) + '\n' for r in cap_rows())
    p = subprocess.run([exe], input=stdin, env=dict(env, **switches), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def cell_diff(cols, base, lines):
    """``lines`` as the cells that differ from ``base``, lines with the same cells together:
    '<line>,<first>-<last>,...: <column>=<value> ...'."""
    out = {}
    for i, (b, g) in enumerate(zip(base, lines)):
        if b != g:
            cells = ' '.join('{}={}'.format(c, y) for c, x, y in zip(cols, b.split(), g.split()) if x != y)
            runs = out.setdefault(cells, [])
            if runs and runs[-1][1] == i - 1:
                runs[-1][1] = i
            else:
                runs.append([i, i])
    return [','.join(str(a) if a == b else '{}-{}'.format(a, b) for a, b in runs) + ': ' + cells
            for cells, runs in out.items()]


def read_golden():
    """set name -> its table's lines (without the header), the cell differences applied to the default."""
    with open(GOLDEN) as f:
        sections = f.read().split('== ')[1:]
    parts = {sec.split('\n', 1)[0]: sec.split('\n', 1)[1].splitlines() for sec in sections}
    cols, base = parts['default'][0].split(), parts['default'][1:]
    tables = {'default': base}
    for name, diffs in parts.items():
        if name != 'default':
            lines = [b.split() for b in base]
            for d in diffs:
                where, cells = d.split(': ')
                for run in where.split(','):
                    for i in range(int(run.split('-')[0]), int(run.split('-')[-1]) + 1):
                        for cell in cells.split():
                            lines[i][cols.index(cell.split('=')[0])] = cell.split('=')[1]
            tables[name] = [' '.join(x) for x in lines]
    return tables


def write_golden():
    cc = _hipcc()
    exe = GOLDEN + '.tmp'
    subprocess.check_call([cc, '--cuda-host-only', '-std=c++17', '-O0', os.path.join(REPO, 'tools', 'route_table.cpp'),
                           '-o', exe])
    try:
        out = {name: run_table(exe, sw).splitlines() for name, sw in SWITCH_SETS.items()}
    finally:
        os.remove(exe)
    base = out['default']
    with open(GOLDEN, 'w') as f:
        f.write('== default\n' + '\n'.join(base) + '\n')
        for name, lines in out.items():
            if name != 'default':
                assert lines[0] == base[0] and len(lines) == len(base)
                f.write('== {}\n'.format(name) + ''.join(d + '\n' for d in cell_diff(base[0].split(), base[1:], lines[1:])))


def launcher_expressions(k, W, sw, v):
    """What njode_cfg.hip evaluated at fb9bab5, from KArgs fields and pointers, where it now reads the route.
    k: the shape's capability bits, sw: the switch set, v: one line of the table (inputs, Sizing, Route)."""
    want_path, drop, save = bool(v['flags'] & C_RETURN_PATH), bool(v['drop']), bool(v['z.save'])
    # KArgs as prepare() filled it from make_layout() (njode_api.hip:1001-1028, :293-:350): a pointer is
    # non-null where the layout took the buffer
    a_chain = bool(v['z.chain'])                                              # a.chain
    lact = save and bool(v['z.chain'] or v['z.lock_act'])                     # L.lk_act
    dbits_row = bool(v['z.train']) and bool(v['z.chain'] or (save and v['z.lock_act']))   # L.dbits_row (:302, :342)
    dbits = bool(v['z.seg_bits']) or dbits_row                                # L.dbits (:293, :305, :343)
    cdelta, cseg = save and bool(v['z.delta']), save and bool(v['z.delta_seg'])   # L.lk_delta, L.lk_seg
    lock4 = not sw.get('NJODE_LOCK4', '1').startswith('0')                    # njode_cfg.hip:57-63
    bits_off = int(sw.get('NJODE_DROP_BITS_AHEAD', '1')) == 0                 # :256, :443
    e = {}
    # lockstep forward, njode_cfg.hip:460 (matrix cores), :462 / :434 (wave per path), :440 (four-wave tiles)
    if not (v['lock_fwd'] == ODE_MFMA and k['HAS_MFMA_LOCK']):
        e['lock_fwd_kind'] = VALU
    elif k['HAS_CHAIN'] and a_chain and not (want_path and drop):
        e['lock_fwd_kind'] = CHAIN
    elif k['HAS_Q4'] and not want_path and lock4 and (not save or lact):
        e['lock_fwd_kind'] = TILE4
    else:
        e['lock_fwd_kind'] = WAVE1
    # lockstep backward (only ever called for a saving flag set), :551, :489-:504
    if save:
        if not (v['lock_sweep'] == ODE_MFMA and k['HAS_MFMA_SWEEP']):
            e['lock_bwd_kind'] = VALU
        elif k['HAS_CHAIN'] and a_chain:
            e['lock_bwd_kind'] = CHAIN
        elif k['HAS_Q4'] and lock4 and lact:
            e['lock_bwd_kind'] = TILE4
        else:
            e['lock_bwd_kind'] = WAVE1
    # keep bits ahead of the masked tiles, :444
    e['lock_bits_ahead'] = e['lock_fwd_kind'] == TILE4 and drop and dbits and dbits_row and not bits_off
    # segment plan: the implementation after :343, the wave-per-item kernels :295, the tails :296
    seg_ode = ODE_VALU if (v['ode'] == ODE_MFMA and not k['HAS_MFMA']) else v['ode']
    e['seg_ode'] = seg_ode
    seg, mfma = bool(v['seg']), seg_ode == ODE_MFMA
    chain = k['HAS_SEG_CHAIN'] and mfma and bool(v['seg_chain'])
    if seg:
        e['tails_ride'] = bool(v['tails']) and chain
        e['side.tails_side'] = bool(v['tails']) and not chain
        # keep bits ahead of the ODE forward, :262-:264 (side: the call has a helper stream)
        for col, side in (('seg_bits_ahead', False), ('side.seg_bits_ahead', True)):
            if v['seg_chain']:
                bits = drop and dbits
            else:
                bits = drop and k['HAS_SPLIT'] and bool(v['ode_split']) and dbits and not side and not bits_off and \
                    v['n_split_fwd'] == v['n_blocks_fwd']
            e[col] = mfma and bool(bits)
    e['enc_blocks'] = int(sw.get('NJODE_ENC_BLOCKS', 4096))                   # :151
    # waves per block of the wave-per-path kernels, :564-:569
    wpb_env = int(sw.get('NJODE_CHAIN_WPB', 0))
    w = 1
    while w < CHAIN_MAX_WAVES and (v['B'] + w - 1) // w > 256:
        w *= 2
    e['chain_wpb'] = wpb_env if 1 <= wpb_env <= CHAIN_MAX_WAVES else w
    # k_ode_dw_stored runs, :638-:639 (lockstep: a.seg_chain is 0) and, with the encoder's pass, :648-:649
    stored = (k['HAS_CHAIN'] or k['HAS_SEG_CHAIN']) and W < 64 and (a_chain or bool(v['seg_chain'])) and cdelta and \
        cseg and v['dw_pair_blocks'] > 0
    if save:
        e['dw_stored'] = bool(stored)
        if v['dw_enc_fused']:   # (:626: a call that asked for it and did not get it failed)
            assert k['HAS_SEG_CHAIN'] and v['seg_chain'] and stored, v
    return e


def check_line(k, W, sw, v):
    kinds = (v['lock_fwd_kind'], v['lock_bwd_kind'])
    # the dispatch part is admitted by the sizing part
    assert v['admitted'] == 1, v
    assert not v['seg_chain'] or v['z.seg_items'], v
    assert CHAIN not in kinds or v['z.chain'], v
    assert not (v['z.save'] and TILE4 in kinds) or v['z.lock_act'], v
    assert not v['seg_bits_ahead'] or v['z.seg_bits'], v
    assert not v['side.seg_bits_ahead'] or v['z.seg_bits'], v
    assert not v['lock_bits_ahead'] or v['z.lock_bits'], v
    assert not (v['lock_fwd_kind'] == CHAIN and v['drop']) or v['z.lock_bits'], v
    # block counts
    assert v['n_split_blocks'] <= v['n_blocks_bwd'] and v['n_split_fwd'] <= v['n_blocks_fwd'], v
    assert v['n_blocks_bwd'] <= v['z.slab_rows'], v
    assert max(v['rows.ode'], v['rows.enc'], v['rows.dec']) <= v['z.slab_rows'], v
    # a saving forward and its backward: the same family
    if v['z.save']:
        assert v['lock_fwd_kind'] == v['lock_bwd_kind'], v
    for col, want in launcher_expressions(k, W, sw, v).items():
        assert v[col] == int(want), (col, want, v)


@pytest.mark.parametrize('name', list(SWITCH_SETS))
def test_route_table(program, name):
    out = run_table(program, SWITCH_SETS[name])
    lines = out.splitlines()
    cols = lines[0].split()
    rows = cap_rows()
    assert len(lines) > 1 + len(rows)
    for line in lines[1:]:
        v = dict(zip(cols, map(int, line.split())))
        H, W, flags = rows[v['row']][:3]
        check_line(dict(zip(CAP_ORDER, rows[v['row']][3:])), W, SWITCH_SETS[name], v)
    want, lines = read_golden()[name], lines[1:]
    assert len(lines) == len(want), (len(lines), len(want))
    diff = [(i, w, g) for i, (w, g) in enumerate(zip(want, lines)) if w != g]
    assert not diff, 'first differing lines (golden, got):\n' + '\n'.join('{}:\n  {}\n  {}'.format(*d) for d in diff[:5]) \
        + '\ncolumns: ' + ' '.join(cols)
