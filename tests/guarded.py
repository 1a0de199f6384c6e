"""A guard-band arena for the buffers of one C-ABI call (a helper module, not a conftest).

Every buffer of the call under test is carved out of ONE torch allocation:

* a buffer starts 256-byte aligned (what torch's own device pointers are) and has EXACTLY the
  stated length: the guard band behind it starts at the first byte past its end;
* before and behind every buffer lies a guard band of at least ``max(1 MiB, size / 2)`` bytes --
  more than the slack the Python wrapper gives (``0.25 size + 4096``), so that any overrun the
  roomy buffers could have been hiding lands in a guard and never becomes a fault;
* the guard contents are chosen so that a stray READ cannot send a kernel out of bounds:

  ``nan32`` / ``nan64``  quiet NaNs, around float inputs: a value read past the end poisons every
                         result it reaches;
  ``index``              ``base + i % modulo`` around integer inputs: wrong but valid path indices
                         (``base`` 0) and small counts (``base`` 1);
  ``pattern``            ``1 + (i + phase) % 3`` per 32-bit word ``i`` of the arena, around (and, until
                         the call writes it, inside) the workspace, the plan and every output: a
                         valid small index as ``int32``, a finite denormal as a float.  ``phase``
                         0 / 1 gives two different images: a call whose results depend on what
                         lies in or around these buffers gives different bits under the two.

``check()`` names every guard that changed: (buffer name, 'before' | 'after', byte offset of the
first changed byte relative to the START of the buffer -- negative before it, >= its length behind
it).  Works on CPU tensors too (``tests/test_guarded_arena.py``).
"""
import torch

ALIGN = 256
MIN_GUARD = 1 << 20
KINDS = ('nan32', 'nan64', 'index', 'pattern')


def _up(n, m=ALIGN):
    return (n + m - 1) // m * m


def guard_bytes(size):
    return _up(max(MIN_GUARD, (size + 1) // 2))


class Arena:
    def __init__(self, device='cuda', phase=0, min_guard=None):
        self.device, self.phase = torch.device(device), int(phase)
        self.min_guard = min_guard      # (tests of the helper itself: smaller bands)
        self.specs, self.where, self.mem, self.image = [], {}, None, None

    def add(self, name, nbytes, kind='pattern', modulo=3, base=0):
        """Declare a buffer of exactly ``nbytes`` bytes; ``kind``: what its guards (and its own
        bytes until they are written) hold."""
        assert self.mem is None and name not in self.where and kind in KINDS and nbytes >= 0
        self.specs.append((name, int(nbytes), kind, (int(base), max(int(modulo), 1))))
        self.where[name] = None
        return self

    def _guard(self, size):
        if self.min_guard is not None:
            return _up(max(self.min_guard, (size + 1) // 2))
        return guard_bytes(size)

    def _fill(self, words, w0, kind, modulo):
        """The guard image of the 32-bit words [w0, w0 + len(words)) of the arena."""
        n = words.numel()
        i = torch.arange(w0, w0 + n, dtype=torch.int64, device=words.device)
        if kind == 'pattern':
            words.copy_(1 + (i + self.phase) % 3)
        elif kind == 'index':
            words.copy_(modulo[0] + i % modulo[1])
        elif kind == 'nan32':
            words.fill_(0x7FC00000)
        else:   # quiet NaN as float64: low word 0, high word 0x7FF80000 (w0 is even: regions are 256-aligned)
            words.copy_((i % 2) * 0x7FF80000)

    def build(self):
        layout, cur = [], 0
        for name, size, kind, modulo in self.specs:
            g = self._guard(size)
            start = cur + g
            end = _up(start + size) + g
            layout.append((name, cur, start, size, end, kind, modulo))
            self.where[name] = (start, size)
            cur = end
        self.layout = layout
        # (one allocation; the arena begins at its first 256-byte boundary -- on the GPU that is
        # its first byte, the host allocator aligns to less)
        self.raw = torch.empty(max(cur, ALIGN) + ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-self.raw.data_ptr()) % ALIGN
        self.mem = self.raw[shift:shift + max(cur, ALIGN)]
        assert self.mem.data_ptr() % ALIGN == 0
        words = self.mem.view(torch.int32)
        for name, lo, start, size, hi, kind, modulo in layout:
            self._fill(words[lo // 4:hi // 4], lo // 4, kind, modulo)
        self.image = self.mem.clone()
        return self

    # -- the buffers --------------------------------------------------------------------------
    def nbytes(self, name):
        return self.where[name][1]

    def ptr(self, name):
        return self.mem.data_ptr() + self.where[name][0]

    def view(self, name, dtype=torch.uint8, shape=None):
        """The buffer as a tensor of ``dtype`` (its length must be a whole number of elements)."""
        start, size = self.where[name]
        t = self.mem[start:start + size].view(dtype)
        return t if shape is None else t.view(shape)

    def put(self, name, tensor):
        """Copy ``tensor``'s bytes into the buffer, which must have exactly their length."""
        src = tensor.detach().contiguous().reshape(-1).view(torch.uint8)
        start, size = self.where[name]
        assert src.numel() == size, (name, src.numel(), size)
        self.mem[start:start + size].copy_(src)
        return self.ptr(name)

    # -- the guards ---------------------------------------------------------------------------
    def check(self):
        """[(name, side, offset)] of every guard band that no longer holds its image."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        out = []
        for name, lo, start, size, hi, kind, modulo in self.layout:
            for side, a, b in (('before', lo, start), ('after', start + size, hi)):
                if torch.equal(self.mem[a:b], self.image[a:b]):
                    continue
                first = int((self.mem[a:b] != self.image[a:b]).nonzero()[0])
                out.append((name, side, a + first - start))
        return out
