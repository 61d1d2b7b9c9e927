"""scrub_ragged and shard_masks_ragged (include/carbonado_hip_repair.h) against
the independent slice verifier and the C oracle: streams of twelve sizes with
damaged chunks, parents and roots in ONE call.  Which shards of a damaged
level-12 stream may be trusted comes from oracle/pyoracle.py
(authentic_shards), the repaired stream from the C oracle's encode(); mask,
status and bytes are exact.  Good shards -> status: 8 -> 12 (UnnecessaryScrub),
fewer than 4 -> 7 (ZfecError), 4 to 7 -> 0 and the oracle's stream.  Every
output buffer is filled with a sentinel and only the range of a status-0 object
may change; the input must not change; the scratch carries guard bytes past
the length the call is told.  Streams sit at offsets 56 and 8 mod 256."""
import functools
import random
import struct
from typing import NamedTuple

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from oracle import oracle as O
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SENT, GUARD = 0xA5, 0x5C
# C below, at and just past one 4 KiB decode block; one-group streams up to
# spc 8, two groups (the top kernel) from 9; shards over several 64-chunk
# subtrees at 33, 64, 65
SPCS = [1, 2, 3, 4, 5, 8, 9, 13, 16, 33, 64, 65]


class Obj(NamedTuple):
    spc: int
    clean: bytes     # O.encode's stream
    flips: tuple     # (stream offset, xor mask) of every damaged bit
    hash: bytes
    good: frozenset  # the oracle's authentic shards of the damaged stream
    padding: int
    chunk_len: int
    what: str

    @property
    def bad(self) -> bytes:
        return B.apply(self.clean, self.flips)

    @property
    def mask(self) -> int:
        return sum(1 << i for i in self.good)

    @property
    def status(self) -> int:
        return 12 if len(self.good) == 8 else 7 if len(self.good) < 4 else 0

    @property
    def selection(self) -> tuple:  # primaries first, then secondaries, ascending
        return tuple(sorted(self.good)[:4])


def _clean(spc: int, seed):
    """A level-12 stream of N = 8 spc chunks with non-zero zfec padding."""
    d = random.Random(repr(seed)).randbytes(4096 * spc - 37 - spc)
    enc, h, info = O.encode(d, 12)
    assert info["chunk_len"] == 1024 * spc and info["padding_len"] == 37 + spc and len(enc) == 8 + 8192 * spc + 64 * (8 * spc - 1)
    return enc, h, info["padding_len"], info["chunk_len"]


def _obj(spc: int, seed, cases, rng, what: str, memo=None) -> Obj:
    """An object over its own data with one bit flipped in each of `cases`
    ((node number, half) of tests/bao_damage.py)."""
    enc, h, pad, cl = _clean(spc, seed)
    memo = P.bao_prime(enc, h, {} if memo is None else memo)
    nodes = B.tree_nodes(8192 * spc)
    flips = tuple(B.pick(nodes, c, rng) for c in cases)
    good = P.authentic_shards(B.apply(enc, flips), h, spc, memo) if flips else set(range(8))
    return Obj(spc, enc, flips, h, frozenset(good), pad, cl, what)


@functools.lru_cache(maxsize=None)
def main_objects() -> tuple:
    """Per size: a flipped bit in one chunk of each shard in turn, in a level-1
    parent, in the root node, and none; for spc = 2 all 256 sets of damaged
    shards.  Every object over its own data, so a row landing on another
    object shows."""
    objs = []
    for spc in SPCS:
        rng = random.Random(f"ragged{spc}")
        nodes = B.tree_nodes(8192 * spc)
        chunks = [k for k, nd in enumerate(nodes) if not nd.parent]
        level1 = [k for k, nd in enumerate(nodes) if nd.level == 1]
        for i in range(8):
            objs.append(_obj(spc, ("shard", spc, i), [(chunks[i * spc + rng.randrange(spc)], -1)], rng, f"shard {i}"))
        objs.append(_obj(spc, ("l1", spc), [(rng.choice(level1), rng.randrange(2))], rng, "level-1 parent"))
        objs.append(_obj(spc, ("root", spc), [(0, rng.randrange(2))], rng, "root"))
        objs.append(_obj(spc, ("none", spc), [], rng, "none"))
        assert nodes[0].parent and (nodes[0].lo, nodes[0].hi) == (0, 8 * spc)
    spc, rng = 2, random.Random("masks")
    chunks = [k for k, nd in enumerate(B.tree_nodes(8192 * spc)) if not nd.parent]
    for m in range(256):
        cases = [(chunks[i * spc + rng.randrange(spc)], -1) for i in range(8) if not m >> i & 1]
        o = _obj(spc, ("mask", m), cases, rng, f"mask {m:#04x}")
        assert o.mask == m  # the oracle's verdict is the mask the damage was built from
        objs.append(o)
    return tuple(objs)


class Result(NamedTuple):
    status: np.ndarray
    out: np.ndarray      # the whole output buffer afterwards
    off: list            # where each stream sits (input and output alike)


def _place(objs):
    """Offsets of the streams in one flat buffer: 56 and 8 mod 256 in turn."""
    off, cur = [], 0
    for j, o in enumerate(objs):
        off.append(cur + (56 if j % 2 == 0 else 8))
        cur = -(-(off[-1] + len(o.clean) + 24) // 256) * 256
    return off, cur


def _hashes(objs, hashes=None):
    import torch
    h = np.frombuffer(b"".join(o.hash for o in objs), dtype=np.uint8).reshape(len(objs), 32).copy()
    for j, x in (hashes or {}).items():
        h[j] = np.frombuffer(x, dtype=np.uint8)
    return torch.from_numpy(h).cuda()


def _input(objs, streams=None):
    off, total = _place(objs)
    host = np.full(total, SENT, dtype=np.uint8)
    for j, o in enumerate(objs):
        s = (streams or {}).get(j, o.bad)
        host[off[j]:off[j] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return host, off, total


def _scratch(in_len, nrepair):
    """The call's scratch as a view of exactly the stated length, guard bytes behind it."""
    import torch
    from carbonado_amd import device as D
    need = D.scrub_ragged_scratch(in_len, nrepair).numel()
    full = torch.full((need + 256,), GUARD, dtype=torch.uint8, device="cuda")
    return full, full[:need]


def _scrub(objs, nrepair=None, padding=None, chunk_len=None, hashes=None, streams=None, in_place=False) -> Result:
    """One scrub_ragged call over `objs` (overrides: {object: value}); checks
    what must not change and returns statuses and the output buffer."""
    import torch
    from carbonado_amd import device as D
    host, off, total = _input(objs, streams)
    in_len = [len(o.clean) for o in objs]
    pads = [(padding or {}).get(j, o.padding) for j, o in enumerate(objs)]
    cls = [(chunk_len or {}).get(j, o.chunk_len) for j, o in enumerate(objs)]
    inp = torch.from_numpy(host).cuda()
    out = inp if in_place else torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    full, scratch = _scratch(in_len, nrepair)
    status = D.scrub_ragged(inp, off, in_len, _hashes(objs, hashes), pads, cls, out, off, scratch)
    torch.cuda.synchronize()
    assert (full[scratch.numel():] == GUARD).all().item(), "bytes past scratch_len were written"
    if not in_place:
        assert np.array_equal(inp.cpu().numpy(), host), "scrub_ragged changed its input"
    return Result(status, out.cpu().numpy(), off)


def _check_rows(objs, res: Result, want_status, before=None):
    """Statuses as expected; a status-0 range is the clean stream, every other
    byte is what it was (`before`: the sentinel, or the input when in place)."""
    assert res.status.tolist() == list(want_status), [
        (j, objs[j].spc, objs[j].what, sorted(objs[j].good), int(res.status[j]), w)
        for j, w in enumerate(want_status) if res.status[j] != w][:8]
    expect = np.full(res.out.size, SENT, dtype=np.uint8) if before is None else before.copy()
    for j, o in enumerate(objs):
        if want_status[j] == 0:
            expect[res.off[j]:res.off[j] + len(o.clean)] = np.frombuffer(o.clean, dtype=np.uint8)
    if not np.array_equal(res.out, expect):
        at = int(np.flatnonzero(res.out != expect)[0])
        j = max(k for k in range(len(objs)) if res.off[k] - 56 <= at)
        raise AssertionError(f"output differs at byte {at}: object {j} (spc {objs[j].spc}, {objs[j].what}, "
                             f"status {want_status[j]}), {at - res.off[j]} bytes into its range")


@functools.lru_cache(maxsize=None)
def main_result() -> Result:
    objs = main_objects()
    return _scrub(objs, nrepair=len(objs))


def test_every_size_and_damage_in_one_call(gpu):
    objs = main_objects()
    assert len(objs) == 11 * len(SPCS) + 256
    want = [o.status for o in objs]
    # nothing vacuous: all three statuses, all 70 four-share selections, both offsets
    assert {0, 7, 12} == set(want)
    assert len({o.selection for o in objs if o.status == 0}) == 70
    assert len({o.clean for o in objs}) == len(objs)
    for spc in SPCS:
        mine = [o for o in objs if o.spc == spc and not o.what.startswith("mask")]
        assert [o.status for o in mine[:8]] == [0] * 8 and [sorted(set(range(8)) - o.good) for o in mine[:8]] == [[i] for i in range(8)]
        assert mine[9].status == 7 and not mine[9].good and mine[10].status == 12
        assert mine[8].status in (0, 7) and len(mine[8].good) < 8
    res = main_result()
    assert {x % 256 for x in res.off} == {56, 8}
    _check_rows(objs, res, want)


def test_many_passes_give_the_same(gpu):
    """nrepair = 1: the least scratch a call accepts, so the repairs take many
    passes; statuses and every byte as with one pass."""
    from carbonado_amd import device as D
    objs = main_objects()
    in_len = [len(o.clean) for o in objs]
    one, least = D.scrub_ragged_scratch(in_len, len(objs)).numel(), D.scrub_ragged_scratch(in_len, 1).numel()
    assert least < one / 10  # (so: more than 10 passes)
    res = _scrub(objs, nrepair=1)
    ref = main_result()
    assert res.status.tolist() == ref.status.tolist() and np.array_equal(res.out, ref.out)


def test_in_place(gpu):
    """d_out is d_in, out_off == in_off: repaired streams are clean afterwards,
    unrepairable and intact ones bit-identical to their input."""
    objs = [o for o in main_objects() if not o.what.startswith("mask")]
    objs += [o for o in main_objects() if o.what.startswith("mask")][::5]
    before, _, _ = _input(objs)
    res = _scrub(objs, in_place=True)
    want = [o.status for o in objs]
    assert {0, 7, 12} == set(want)
    _check_rows(objs, res, want, before=before)


def _small_set():
    """A few objects of five sizes, each repairable, from the main set."""
    pick = [o for o in main_objects() if o.spc in (2, 3, 5, 9, 33) and o.what in ("shard 1", "shard 6")]
    assert len(pick) == 10 and all(o.status == 0 for o in pick)
    return pick


def test_per_object_errors_leave_the_neighbours_alone(gpu):
    objs = _small_set()
    clean = {j: o.clean for j, o in enumerate(objs)}
    (n,) = struct.unpack("<Q", objs[6].clean[:8])
    bad_hash = bytes([objs[7].hash[0] ^ 1]) + objs[7].hash[1:]
    over = dict(
        padding={1: objs[1].padding + 4096,   # recomputed padding differs -> 13
                 2: objs[2].padding + 1},     # consistent, but another object: its hash differs -> 15
        chunk_len={3: 0, 4: objs[4].chunk_len + 1024, 5: objs[5].chunk_len + 7},
        streams={6: struct.pack("<Q", n + 1) + objs[6].bad[8:], 7: clean[7]},
        hashes={7: bad_hash})
    assert objs[1].chunk_len >= 2048 and objs[1].padding + 4096 <= 4 * objs[1].chunk_len
    want = [0, 13, 15, 7, 7, 7, 7, 7, 0, 0]
    res = _scrub(objs, **over)
    _check_rows(objs, res, want)
    # the masks behind them: a chunk_len that does not fit, a header off by one and a wrong hash leave no shard
    masks = _masks(objs, chunk_len=over["chunk_len"], streams=over["streams"], hashes=over["hashes"])
    assert masks[3:8] == [0] * 5 and masks[:3] == [o.mask for o in objs[:3]] and masks[8:] == [o.mask for o in objs[8:]]


def test_isolation(gpu):
    """Damage to one stream changes neither the status nor the bytes of another."""
    objs = _small_set()
    a = _scrub(objs)
    b = _scrub(objs, streams={4: objs[4].clean})  # object 4 intact
    flips = ((8 + 3, 0x10),)  # object 4's root node (the first after the header) damaged: unrepairable
    c = _scrub(objs, streams={4: B.apply(objs[4].clean, flips)})
    assert a.status.tolist() == [0] * 10 and b.status[4] == 12 and c.status[4] == 7
    lo, hi = a.off[4] - 56, a.off[5] - 56
    for other in (b, c):
        assert np.delete(other.status, 4).tolist() == [0] * 9
        assert np.array_equal(other.out[:lo], a.out[:lo]) and np.array_equal(other.out[hi:], a.out[hi:])
        assert (other.out[lo:hi] == SENT).all()


@pytest.mark.parametrize("spc", [3, 9, 33])
def test_agrees_with_the_uniform_call(gpu, spc):
    """device.scrub_batch on the same damaged streams: the same statuses and rows."""
    import torch
    from carbonado_amd import device as D
    everything, res = main_objects(), main_result()
    idx = [j for j, o in enumerate(everything) if o.spc == spc]
    objs = [everything[j] for j in idx]
    L, count = len(objs[0].clean), len(objs)
    stride = (56 + L + 15) // 16 * 16 + 16
    host = np.full((count, stride), SENT, dtype=np.uint8)
    for r, o in enumerate(objs):
        host[r, 56:56 + L] = np.frombuffer(o.bad, dtype=np.uint8)
    out = torch.full((count, stride), SENT, dtype=torch.uint8, device="cuda")
    status = D.scrub_batch(torch.from_numpy(host).cuda(), L, _hashes(objs), objs[0].padding, objs[0].chunk_len, out,
                           D.scrub_scratch(L, count), offset=56)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert status.tolist() == [int(res.status[j]) for j in idx] and {0, 7, 12} == set(status.tolist())
    for r, j in enumerate(idx):
        assert np.array_equal(got[r, 56:56 + L], res.out[res.off[j]:res.off[j] + L]), (spc, objs[r].what)


def _masks(objs, chunk_len=None, streams=None, hashes=None):
    """shard_masks_ragged alone: the masks; nothing but them and the scratch written."""
    import torch
    from carbonado_amd import device as D
    host, off, _ = _input(objs, streams)
    in_len = [len(o.clean) for o in objs]
    cls = [(chunk_len or {}).get(j, o.chunk_len) for j, o in enumerate(objs)]
    inp = torch.from_numpy(host).cuda()
    full, scratch = _scratch(in_len, 1)
    masks = torch.full((len(objs) + 8,), -1, dtype=torch.int32, device="cuda")
    got = D.shard_masks_ragged(inp, off, in_len, _hashes(objs, hashes), cls, scratch, masks=masks)
    torch.cuda.synchronize()
    assert got is masks and (masks[len(objs):] == -1).all().item()
    assert (full[scratch.numel():] == GUARD).all().item(), "bytes past scratch_len were written"
    assert np.array_equal(inp.cpu().numpy(), host), "shard_masks_ragged changed its input"
    return masks[:len(objs)].tolist()


def test_shard_masks_alone(gpu):
    objs = main_objects()
    got = _masks(objs)
    want = [o.mask for o in objs]
    assert got == want, [(j, objs[j].spc, objs[j].what, hex(got[j]), hex(want[j])) for j in range(len(objs))
                         if got[j] != want[j]][:8]
    assert set(range(256)) <= set(want)


def test_one_16_mib_object(gpu):
    """N = 32768 chunks, the largest stream a call takes: a damaged primary
    shard is decoded from three primaries and a secondary and re-encoded."""
    spc = 4096
    d = np.random.default_rng(16).integers(0, 256, (16 << 20) - 41, dtype=np.uint8).tobytes()
    enc, h, info = O.encode(d, 12)
    assert info["chunk_len"] == 1024 * spc and info["padding_len"] == 41
    nodes = B.tree_nodes(8192 * spc)
    k = next(j for j, nd in enumerate(nodes) if not nd.parent and nd.lo == spc + 1234)
    flips = (B.pick(nodes, (k, -1), random.Random(16)),)
    good = P.authentic_shards(B.apply(enc, flips), h, spc, P.bao_prime(enc, h))
    o = Obj(spc, enc, flips, h, frozenset(good), info["padding_len"], info["chunk_len"], "shard 1")
    assert o.mask == 0xFD and o.selection == (0, 2, 3, 4)
    _check_rows([o], _scrub([o]), [0])
