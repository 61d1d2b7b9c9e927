"""A flat device buffer that reaches past 4 GiB, for the tests that place what
a device call reads or writes at offsets and pitches of 2^32 and more
(tests/test_gpu_far_offsets.py).

A compact image (a test's streams, inputs or outputs at offsets from 0) is
moved to BASE(cut) = 2^32 - cut: compact position `cut` is then byte 2^32 of
the buffer, and every offset of the compact layout becomes BASE + off.  cut is
a multiple of 256, so every 16-byte and 256-byte residue and every
STREAM_OFFSET phase of the compact layout survives the shift.

An offset that lost its upper bits on the way to a lane's address does not
fault: the write lands 4 GiB lower, in [0, S) of the same buffer.  So the
buffer is filled with a canary once, a test names the windows it may write,
and untouched_outside() checks every other byte on the device."""
import numpy as np

FOUR_GIB = 1 << 32
CANARY = 0xC7          # the canary of read_world.py: a far content buffer is a canary-filled one
PIECE = 256 << 20      # bytes compared at once in untouched_outside()


def BASE(cut: int) -> int:
    assert cut % 256 == 0 and 0 <= cut <= FOUR_GIB
    return FOUR_GIB - cut


def cut_for(off: int, length: int) -> int:
    """The cut that puts byte 2^32 in the middle of the compact range [off, off + length)."""
    return (off + length // 2) // 256 * 256


def placement(base: int, offs, lens):
    """(below, straddling, above): the indices of the ranges [base + off, base + off + len)
    that lie entirely below 2^32, contain bytes 2^32 - 1 and 2^32, or lie entirely above."""
    below, across, above = [], [], []
    for i, (o, n) in enumerate(zip(offs, lens)):
        a, b = base + o, base + o + n
        (below if b <= FOUR_GIB else above if a >= FOUR_GIB else across).append(i)
    return below, across, above


def assert_straddles(base: int, offs, lens, named: int, side: int = 1024):
    """The placement every far test asserts first: something entirely below
    2^32, exactly the named range across it with `side` bytes on each side,
    something entirely above."""
    below, across, above = placement(base, offs, lens)
    assert below and above, (below, across, above)
    assert across == [named], (across, named)
    a, n = base + offs[named], lens[named]
    assert FOUR_GIB - a >= side and a + n - FOUR_GIB >= side, (a, n, side)


class Far:
    """One flat uint8 device buffer of 2^32 + room bytes, canary-filled."""

    def __init__(self, room: int):
        import torch
        self.torch = torch
        self.size = FOUR_GIB + room
        self.buf = torch.empty(self.size, dtype=torch.uint8, device="cuda")
        self.buf.fill_(CANARY)
        torch.cuda.synchronize()
        self.used = []  # (start, size) of every range a test put, looked at or named as a window

    def _note(self, a: int, n: int):
        self.used.append((max(0, a), n))

    def put(self, image, base: int):
        """Upload a compact image (numpy uint8, or a device tensor) to [base, base + len)."""
        torch = self.torch
        t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.array(image, dtype=np.uint8))
        assert base >= 0 and base + t.numel() <= self.size
        self._note(base, t.numel())
        self.buf[base:base + t.numel()].copy_(t.reshape(-1))

    def window(self, base: int, size: int, guard: int = 0) -> np.ndarray:
        """[base - guard, base + size + guard) on the host."""
        assert base - guard >= 0 and base + size + guard <= self.size
        self._note(base - guard, size + 2 * guard)
        return self.buf[base - guard:base + size + guard].cpu().numpy()

    def _outside(self, windows):
        """the gaps between the windows [(start, size)], in pieces of at most PIECE bytes"""
        at = 0
        for a, n in sorted((int(a), int(n)) for a, n in windows if n):
            assert 0 <= a and a + n <= self.size
            for p in range(at, a, PIECE):
                yield p, min(a, p + PIECE)
            at = max(at, a + n)
        for p in range(at, self.size, PIECE):
            yield p, min(self.size, p + PIECE)

    def untouched_outside(self, windows) -> bool:
        """Every byte outside the windows [(start, size)] still holds the
        canary.  Compared on the device piece by piece; one word comes back."""
        torch = self.torch
        for a, n in windows:
            self._note(int(a), int(n))
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for a, b in self._outside(windows):
            bad += (self.buf[a:b] != CANARY).sum()
        return int(bad.item()) == 0

    def first_touched(self, windows):
        """For a failure's message: the first byte outside the windows that lost its canary, or None."""
        for a, b in self._outside(windows):
            hit = self.torch.nonzero(self.buf[a:b] != CANARY)
            if hit.numel():
                return a + int(hit[0])
        return None

    def refill(self, windows, low: int = 0):
        """Canary back into the windows a test used and into the low region [0, low)."""
        for a, n in list(windows) + [(0, low)]:
            self.buf[max(0, int(a)):min(self.size, int(a) + int(n))].fill_(CANARY)
        self.torch.cuda.synchronize()

    def reset(self, guard: int = 4096):
        """After every test, passed or failed: the canary back into whatever it
        used and into the low region a narrowed offset of it would have hit, so
        that one failure does not show again in the tests behind it.  Never the
        whole buffer."""
        if self.buf is None or not self.used:
            return
        longest = max(n for _, n in self.used)
        self.refill([(a - guard, n + 2 * guard) for a, n in self.used], low=longest + 2 * guard)
        self.used = []
