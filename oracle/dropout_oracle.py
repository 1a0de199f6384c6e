"""
TEST INFRASTRUCTURE (oracle/): numpy restatement of the dropout keep-bit stream of the
matrix-core kernels (njode_amd/csrc/njode_device.h: fmix32, drop_state; njode_mfma.h:
keep_bits).  Only tests/ may import it.

The reference draws its masks with torch's bernoulli_ (models.py:148-160, nn.Dropout), which a
GPU kernel cannot reproduce bit for bit; parity of the dropout path is therefore statistical
(SURVEY.md section 7).  This file pins WHAT the kernels draw, so that the stream itself can be
tested: keep rate per unit, independence across units / Euler steps / paths / networks.

Stream of one network evaluation for lane group g (the lanes holding units 4q + g of the
wave's 16 chains):  state = drop_state(seed, gid, gid_hi + 0x5bd1e995 (g + 1), tkey, net);
word i = i-th xorshift32 (13, 17, 5) output; unit 4q + g of hidden layer 1 is kept iff the
(q & 1 ? high : low) 16 bits of word q >> 1 are >= thr16 = round(p 65536); layer 2 continues
the stream after ceil(Q / 2) words.

The kernels draw from three word streams.  All start from drop_state(seed, gid, tkey, net), the
call seed being models.py's (dropout_seed * 0x9E3779B97F4A7C15 + step) mod 2^64, gid the GLOBAL
path id (NjodeBatch.path_id_offset + b, 64-bit):

  'mc'    matrix-core lane groups (keep_units above; njode_mfma.h keep_bits, row_keep_bits,
          chain_masks, q4_row_keep / q4_ode_keep).  Q = registers per lane: (W + 4) / 4 for the
          ODE net (MF<C>::Q1), 16 for the encoder and readout (the row kernels' keep_bits<16>).
  'valu'  one xorshift32 state per evaluation (njode_kernels.h Masks::draw, keep_mask<W>):
          unit u of hidden layer 1 is the (u & 1 ? high : low) half of word u >> 1; layer 2
          continues the same state after ceil(W / 2) words.
  'gen'   one fmix32 per unit pair (njode_gen.h drop_base / drop_word): word of (layer l, pair
          j) = fmix32(state ^ (l 0x9e3779b9 + j 0x85ebca6b + 0x632be5ab)), unit 2j low half,
          2j + 1 high half; every hidden layer l = 0 .. depth - 1 has its own words.

Which stream each kernel of each route draws, per network (ODE: the Euler step's ODE net; ENC:
the encoder at the start and at a jump; DEC_BJ / DEC: the readout before / after a jump; ROW:
the readout of a path-output row):

  route (kernels)                                            ODE         ENC, DEC_BJ, DEC, ROW
  wave per item (k_seg_fwd_chain / k_seg_bwd_chain)          mc, Q1      mc, 16
  split, mixed (k_ode_{fwd,bwd}_mixed)                       mc, Q1      mc, 16
  one wave (k_ode_{fwd,bwd}_mfma, k_*_rows_mfma)             mc, Q1      mc, 16
  lockstep (k_paths_fwd_mfma, k_paths_bwd_adj_mfma)          mc, Q1      mc, 16
  four-wave lockstep (k_paths_fwd_mfma + lock4 backward)     mc, Q1      mc, 16
  wave per path (k_chain_bits copies, k_paths_*_chain)       mc, Q1      mc, 16
  VALU (NJODE_ODE=valu: k_ode_*_items, k_*_rows; k_paths_*;
        use_rnn shapes: k_paths_fwd, k_paths_bwd_adj)        valu        valu
  shape-generic (k_gen_*, k_gseg_*)                          gen         gen

Time keys (njode_kernels.h:14-15, njode_gen.h:43-44): the Euler step index k for the ODE net;
k_jump[i] (Euler steps completed when jump i happens) for the encoder and both readouts of a
jump; TKEY_START for the start encoding; TKEY_START - 1 for the first path-output row and
0x80000000 + k for the row after Euler step k.  Nets: ODE 0, ENC 1, DEC 2, DEC_BJ 3, ROW 4.

Threshold and scale are the kernels' (njode_api.hip, njode_gen.hip), not torch's:
thr16 = (unsigned)(fp32(p) 65536 + 0.5f) clamped to 65535, and a kept unit is multiplied by the
fp32 value 1 / (1 - thr16 / 65536) -- not by 1 / (1 - p); the two differ by up to ~7.6e-5
relative at p = 0.9.  A call whose networks have no hidden layer draws no mask (thr16 = 0).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
NET_ODE, NET_ENC, NET_DEC, NET_DEC_BJ, NET_DEC_ROW = 0, 1, 2, 3, 4
TKEY_START = 0xFFFFFFFF
STREAMS = ('mc', 'valu', 'gen')


def thr16(p):
    """The kernels' drop threshold: (unsigned)(p * 65536.0f + 0.5f) in fp32, clamped to 65535."""
    t = int(np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5))
    return min(t, 65535)


def inv_keep(p):
    """The kernels' inverted-dropout factor (fp32): 1 / (1 - thr16 / 65536)."""
    keep = np.float32(1.0) - np.float32(thr16(p)) / np.float32(65536.0)
    return float(np.float32(1.0) / keep)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def fmix32(h):
    h = _u32(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def drop_state(seed, gid_lo, gid_hi, tkey, net):
    seed_lo, seed_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    gid_lo, gid_hi, tkey, net = _u32(gid_lo), _u32(gid_hi), _u32(tkey), _u32(net)
    h = fmix32(seed_lo ^ ((gid_lo * np.uint64(0x9e3779b9)) & M32))
    h = fmix32(h ^ seed_hi ^ ((gid_hi * np.uint64(0x7f4a7c15)) & M32)
               ^ ((tkey * np.uint64(0x85ebca6b)) & M32))
    h = fmix32(h ^ ((net * np.uint64(0xc2b2ae35)) & M32) ^ np.uint64(0x27d4eb2f))
    return np.where(h == 0, np.uint64(0x9e3779b9), h)


def xorshift32_words(state, n):
    """n successive outputs of xorshift32 (13, 17, 5) for every state (vectorised);
    returns [n, ...]."""
    s = _u32(state).copy()
    out = []
    for _ in range(n):
        s ^= (s << np.uint64(13)) & M32
        s ^= s >> np.uint64(17)
        s ^= (s << np.uint64(5)) & M32
        out.append(s.copy())
    return np.stack(out)


def mfma_group_state(seed, gid, g, tkey, net):
    gid = np.asarray(gid, dtype=np.uint64)
    hi = ((gid >> np.uint64(32)) + np.uint64(0x5bd1e995) * np.uint64(g + 1)) & M32
    return drop_state(seed, gid & M32, hi, tkey, net)


def keep_units(seed, gid, tkey, net, width, p, layer=0, nq=None):
    """0/1 keep indicators [..., width] of hidden layer `layer` (0 or 1) of one network
    evaluation, as the matrix-core kernels draw them.  nq: registers per lane of the draw
    (default (width + 4) / 4, the ODE net's; the encoder and readout draw 16)."""
    thr = np.uint64(thr16(p))
    q_regs = (width + 1 + 3) // 4               # registers per lane (units + bias unit)
    n_words = ((q_regs if nq is None else nq) + 1) // 2
    gid = np.asarray(gid, dtype=np.uint64)
    keep = np.zeros(gid.shape + (width,), dtype=np.uint8)
    for g in range(4):
        st = mfma_group_state(seed, gid, g, tkey, net)
        words = xorshift32_words(st, 2 * n_words)[layer * n_words:(layer + 1) * n_words]
        for q in range(q_regs):
            u = 4 * q + g
            if u >= width:
                continue
            w = words[q >> 1]
            bits = (w >> np.uint64(16)) if (q & 1) else (w & np.uint64(0xFFFF))
            keep[..., u] = (bits >= thr).astype(np.uint8)
    return keep


def _halves(words, width, thr):
    """[..., n_words] words -> [..., width] keep bits: unit 2j low half, 2j + 1 high half of word j."""
    lo, hi = words & np.uint64(0xFFFF), words >> np.uint64(16)
    bits = np.stack([lo, hi], axis=-1).reshape(words.shape[:-1] + (2 * words.shape[-1],))[..., :width]
    return (bits >= np.uint64(thr)).astype(np.uint8)


def path_state(seed, gid, tkey, net):
    """drop_state of a 64-bit global path id (the VALU and generic streams: no lane-group offset)."""
    gid = np.asarray(gid, dtype=np.uint64)
    return drop_state(seed, gid & M32, gid >> np.uint64(32), tkey, net)


def valu_keep(seed, gid, tkey, net, width, p, layer=0):
    """Keep indicators [..., width] of hidden layer `layer` (0 or 1) as the VALU kernels draw them
    (njode_device.h keep_mask<W>, njode_kernels.h Masks::draw): layer 2 continues layer 1's state."""
    n_words = (width + 1) // 2
    words = xorshift32_words(path_state(seed, gid, tkey, net), (layer + 1) * n_words)[layer * n_words:]
    return _halves(np.moveaxis(words, 0, -1), width, thr16(p))


def gen_word(base, layer, pair):
    """njode_gen.h drop_word: fmix32(base ^ (layer 0x9e3779b9 + pair 0x85ebca6b + 0x632be5ab))."""
    k = (np.uint64(layer) * np.uint64(0x9e3779b9) + np.asarray(pair, dtype=np.uint64) * np.uint64(0x85ebca6b)
         + np.uint64(0x632be5ab)) & M32
    return fmix32(_u32(base) ^ k)


def gen_keep(seed, gid, tkey, net, width, p, layer=0):
    """Keep indicators [..., width] of hidden layer `layer` (any depth) as the shape-generic kernels
    draw them (njode_gen.h drop_base / drop_word)."""
    base = path_state(seed, gid, tkey, net)
    pairs = np.arange((width + 1) // 2, dtype=np.uint64)
    return _halves(gen_word(base[..., None], layer, pairs), width, thr16(p))


def keep_mask(stream, seed, gid, tkey, net, layer, width, p):
    """The keep indicators [..., width] a kernel family draws for hidden layer `layer` of network
    `net` at time key `tkey` (module docstring: the key schedule)."""
    if stream == 'mc':
        return keep_units(seed, gid, tkey, net, width, p, layer, nq=None if net == NET_ODE else 16)
    if stream == 'valu':
        return valu_keep(seed, gid, tkey, net, width, p, layer)
    if stream == 'gen':
        return gen_keep(seed, gid, tkey, net, width, p, layer)
    raise ValueError(stream)


class KernelMasks:
    """Mask source of the float64 oracle (njode_oracle.OracleNJODE.masks): the keep masks one kernel
    family draws for one call.  ``gid0``: NjodeBatch.path_id_offset of the batch (row b is global
    path gid0 + b); ``seed``: the call seed.  ``__call__(net, tkey, rows, layer, width)`` returns the
    [len(rows), width] keep indicators; ``scale`` is the kernels' fp32 inverted-dropout factor."""

    def __init__(self, stream, seed, p, gid0=0):
        if stream not in STREAMS:
            raise ValueError(stream)
        self.stream, self.seed, self.p, self.gid0 = stream, int(seed), float(p), int(gid0)
        self.scale = inv_keep(p)
        self._cache = {}

    def __call__(self, net, tkey, rows, layer, width):
        rows = np.asarray(rows, dtype=np.uint64)
        key = (net, int(tkey), rows.tobytes(), layer, width)
        if key not in self._cache:
            gid = rows + np.uint64(self.gid0)
            self._cache[key] = keep_mask(self.stream, self.seed, gid, np.uint64(tkey), net, layer, width, self.p)
        return self._cache[key]


def call_seed(dropout_seed, step):
    """models.py: the seed of a training call, (dropout_seed * 0x9E3779B97F4A7C15 + step) mod 2^64."""
    return (int(dropout_seed) * 0x9E3779B97F4A7C15 + int(step)) & 0xFFFFFFFFFFFFFFFF
