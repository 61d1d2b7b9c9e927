"""scrub, scrub_batch and verify_slice against an independent bao slice
verifier.  Which shards of a damaged level-12 stream may be trusted comes from
oracle/pyoracle.py (authentic_shards: bao's SliceDecoder restated, pinned by
tests/test_slice_verify.py), the repaired stream from the C oracle's encode();
status, mask and bytes are exact.  Good shards -> status: 8 -> 12
(UnnecessaryScrub), fewer than 4 -> 7 (ZfecError), 4 to 7 -> 0 and the
oracle's stream.  Every batch call gets `out` filled with a sentinel, and only
the L bytes of a status-0 row may change; each batch test runs with the
streams at offset 0 and 56 of their rows."""
import functools
import random
import struct
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from oracle import oracle as O
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SENT = 0xA5


class Case(NamedTuple):
    clean: bytes        # O.encode's stream
    flips: tuple        # (stream offset, xor mask) of every damaged bit
    hash: bytes
    good: frozenset     # the oracle's authentic shards of the damaged stream
    what: tuple         # the damage, for a failure message

    @property
    def bad(self) -> bytes:
        return B.apply(self.clean, self.flips)

    @property
    def status(self) -> int:
        return 12 if len(self.good) == 8 else 7 if len(self.good) < 4 else 0


class Group(NamedTuple):
    spc: int
    L: int
    info: SimpleNamespace  # padding_len, chunk_len (one EncodeInfo per size)
    cases: list


def _clean(spc: int, seed):
    """A level-12 stream of N = 8 spc chunks with non-zero zfec padding."""
    d = random.Random(repr(seed)).randbytes(4096 * spc - 37 - spc)
    enc, h, info = O.encode(d, 12)
    assert info["chunk_slice_count"] == spc and info["chunk_len"] == 1024 * spc and info["padding_len"] == 37 + spc
    return enc, h, SimpleNamespace(padding_len=info["padding_len"], chunk_len=info["chunk_len"])


def _group(spc: int, kind: str, damages, distinct=True) -> Group:
    """One Case per entry of `damages` (a function of the node list giving
    lists of (node, half) to flip), each over its own data unless `distinct`
    is off (the 4 MiB streams: one clean stream per size)."""
    nodes = B.tree_nodes(8192 * spc)
    cases, memo, shared = [], {}, None
    rng = random.Random(f"{kind}{spc}")
    for j, dmg in enumerate(damages(nodes)):
        if distinct or shared is None:
            shared = _clean(spc, (kind, spc, j))
            P.bao_prime(shared[0], shared[1], memo)
        enc, h, info = shared
        flips = tuple(B.pick(nodes, c, rng) for c in dmg)
        good = P.authentic_shards(B.apply(enc, flips), h, spc, memo)
        cases.append(Case(enc, flips, h, frozenset(good), tuple(dmg)))
    return Group(spc, len(enc), info, cases)


def _run_batch(g: Group, off: int):
    """scrub_batch of the group's damaged streams `off` bytes into their
    rows: statuses, repaired rows and every byte that must not change."""
    import torch
    from carbonado_amd import device as D
    count, L = len(g.cases), g.L
    stride = (off + L + 15) // 16 * 16 + 16
    host = np.full((count, stride), SENT, dtype=np.uint8)
    hashes = np.empty((count, 32), dtype=np.uint8)
    for o, c in enumerate(g.cases):
        host[o, off:off + L] = np.frombuffer(c.bad, dtype=np.uint8)
        hashes[o] = np.frombuffer(c.hash, dtype=np.uint8)
    inp = torch.from_numpy(host).cuda()
    out = torch.full((count, stride), SENT, dtype=torch.uint8, device="cuda")
    status = D.scrub_batch(inp, L, torch.from_numpy(hashes).cuda(), g.info.padding_len, g.info.chunk_len, out,
                           D.scrub_scratch(L, count), offset=off)
    torch.cuda.synchronize()
    assert np.array_equal(inp.cpu().numpy(), host), "scrub_batch changed its input"
    got = out.cpu().numpy()
    want = [c.status for c in g.cases]
    assert status.tolist() == want, [(o, g.cases[o].what, sorted(g.cases[o].good), int(status[o]), want[o])
                                     for o in range(count) if status[o] != want[o]][:8]
    for o, c in enumerate(g.cases):
        if c.status == 0:
            assert got[o, off:off + L].tobytes() == c.clean, (g.spc, o, c.what, "repaired row differs from the oracle")
            assert (got[o, :off] == SENT).all() and (got[o, off + L:] == SENT).all(), (g.spc, o, c.what)
        else:
            assert (got[o] == SENT).all(), (g.spc, o, c.what, "row written despite status %d" % c.status)
    return status


def _run_single(g: Group, picks):
    """ca.scrub (the host slice walk) on the picked cases: the oracle's status and bytes."""
    import carbonado_amd as ca
    from carbonado_amd.error import CarbonadoError
    for o in picks:
        c = g.cases[o]
        try:
            got, st = ca.scrub(c.bad, c.hash, g.info), 0
        except CarbonadoError as e:
            got, st = None, e.status
        assert st == c.status, (g.spc, o, c.what, sorted(c.good))
        if st == 0:
            assert got == c.clean, (g.spc, o, c.what)


# ---- a. every node, small trees ----------------------------------------------

SMALL = [1, 2, 3, 5, 9, 13]


@functools.lru_cache(maxsize=None)
def every_node(spc: int) -> Group:
    g = _group(spc, "every", lambda nodes: [[c] for c in B.every_node_cases(nodes)])
    N = 8 * spc
    assert len(g.cases) == 2 * (N - 1) + N
    return g


@pytest.mark.parametrize("off", [0, 56])
@pytest.mark.parametrize("spc", SMALL)
def test_batch_every_node(gpu, spc, off):
    """One object per damaged node (each parent's left and right half, each
    chunk), all 2 (N - 1) + N of a size in one call: N = 104 is 310 objects,
    well past the 64-repair group, with mixed share patterns."""
    g = every_node(spc)
    status = _run_batch(g, off)
    assert len(status) == 2 * (8 * spc - 1) + 8 * spc
    # a node below one shard leaves 7, the root and its like leave none
    assert {0, 7} <= set(status.tolist()) and 12 not in status


@pytest.mark.parametrize("spc", SMALL)
def test_single_every_node(gpu, spc):
    """The same cases through scrub(): all of them at N = 8, 16, 24, a seeded 32 above."""
    g = every_node(spc)
    picks = range(len(g.cases)) if spc <= 3 else random.Random(spc).sample(range(len(g.cases)), 32)
    assert len(picks) == (len(g.cases) if spc <= 3 else 32)
    _run_single(g, picks)


# ---- b. all 256 shard masks ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def every_mask(spc: int) -> Group:
    def damages(nodes):
        chunks = [k for k, nd in enumerate(nodes) if not nd.parent]
        rng = random.Random(spc)
        return [[(chunks[i * spc + rng.randrange(spc)], -1) for i in range(8) if not m >> i & 1] for m in range(256)]
    g = _group(spc, "mask", damages)
    assert len(g.cases) == 256
    for m, c in enumerate(g.cases):  # the oracle's verdict is the mask the damage was built from
        assert c.good == {i for i in range(8) if m >> i & 1}, m
    return g


@pytest.mark.parametrize("off", [0, 56])
@pytest.mark.parametrize("spc", [1, 3])
def test_batch_every_shard_mask(gpu, spc, off):
    """Object m has one content bit flipped in each shard whose bit is clear
    in m: all 70 four-share patterns, every choice among 5 to 7 good shares,
    162 repairs (three groups) through the pattern sort, each object over its
    own data so that a row landing on another object shows."""
    g = every_mask(spc)
    status = _run_batch(g, off)
    assert len(status) == 256
    assert (status == 0).sum() == 162 and (status == 7).sum() == 93 and (status == 12).sum() == 1
    assert len({c.clean for c in g.cases}) == 256


# ---- c. large trees, chosen nodes --------------------------------------------

LARGE = [64, 65, 512, 513]
CHOSEN = {64: 35, 65: 73, 512: 41, 513: 100}  # cases per size: power-of-two shards straddle 7 parents, odd ones many


@functools.lru_cache(maxsize=None)
def chosen_nodes(spc: int) -> Group:
    return _group(spc, "chosen", lambda nodes: [[c] for c in B.chosen_node_cases(nodes, spc)], distinct=False)


def _check_chosen(g: Group):
    """The chosen set holds what it is meant to: the root, both ends of every
    level, the 16 shard-edge chunks, and the parents over a shard boundary."""
    spc, N = g.spc, 8 * g.spc
    nodes = B.tree_nodes(8192 * spc)
    picked = {c.what[0][0] for c in g.cases}
    assert len(picked) == len(g.cases)
    spans = {(nodes[k].lo, nodes[k].hi) for k in picked}
    assert (0, N) in spans
    assert {(i * spc, i * spc + 1) for i in range(8)} | {((i + 1) * spc - 1, (i + 1) * spc) for i in range(8)} <= spans
    assert sum(1 for lo, hi in spans if hi - lo == 1) == 16
    straddle = {(nd.lo, nd.hi) for nd in nodes if nd.parent and (nd.hi - 1) // spc > nd.lo // spc}
    assert straddle <= spans
    for lv in range(1, (N - 1).bit_length() + 1):
        at = [(nd.lo, nd.hi) for nd in nodes if nd.level == lv]
        assert at and {at[0], at[-1]} <= spans, lv
    return len(straddle)


@pytest.mark.parametrize("off", [0, 56])
@pytest.mark.parametrize("spc", LARGE)
def test_batch_chosen_nodes_large(gpu, spc, off):
    """N = 512, 520, 4096, 4104 (odd promotions at 520 and 4104; 4104 is past
    the one-pass verify of the single call): the root, the first and last node
    of every level, every parent over a shard boundary, the first and last
    chunk of every shard, one object each, one call per size."""
    g = chosen_nodes(spc)
    nstraddle = _check_chosen(g)
    status = _run_batch(g, off)
    assert len(status) == len(g.cases) == CHOSEN[spc] >= 16 + nstraddle
    assert {0, 7} <= set(status.tolist())


@pytest.mark.parametrize("spc", LARGE)
def test_single_chosen_nodes_large(gpu, spc):
    g = chosen_nodes(spc)
    picks = random.Random(spc).sample(range(len(g.cases)), 8)
    _run_single(g, picks)


# ---- d. several nodes at once -------------------------------------------------

@functools.lru_cache(maxsize=None)
def several_nodes() -> Group:
    def damages(nodes):
        rng = random.Random(104)
        parents = [k for k, nd in enumerate(nodes) if nd.parent]
        chunks = [k for k, nd in enumerate(nodes) if not nd.parent]
        out = []
        for j in range(64):  # one parent and one chunk at least, a third node of either kind for half of them
            ks = [rng.choice(parents), rng.choice(chunks)] + ([rng.choice(parents + chunks)] if j % 2 else [])
            out.append([(k, rng.randrange(2) if nodes[k].parent else -1) for k in ks])
        return out
    g = _group(13, "several", damages)
    assert len(g.cases) == 64 and all(2 <= len(c.what) <= 3 for c in g.cases)
    return g


@pytest.mark.parametrize("off", [0, 56])
def test_batch_several_damaged_nodes(gpu, off):
    """64 objects at N = 104 with two or three damaged nodes each, parents and
    chunks mixed; the mask is the oracle's."""
    g = several_nodes()
    status = _run_batch(g, off)
    assert len(status) == 64 and {0, 7} <= set(status.tolist())
    if off == 0:
        _run_single(g, range(0, 64, 4))


# ---- e. header damage ----------------------------------------------------------

@pytest.mark.parametrize("off", [0, 56])
def test_header_damage_is_refused(gpu, off):
    """A stream whose length header is damaged (one bit: made larger by 1, by
    2^40, made smaller) is never repaired: both calls give a non-zero status
    and the batch writes nothing.  Which status is not pinned; on an MI355X
    the batch gives 7 (ZfecError: a header that is not the expected length
    leaves no shard trusted) for all three, scrub() gives BaoDecodeError
    Truncated (C status 6) for the two enlarged headers, whose stream is
    shorter than they imply, and 7 for the smaller one.  bao itself checks the
    length only through the tree shape: for the header one too large the
    oracle still accepts shards 0 to 4 (the 16-chunk left subtree keeps its
    shape), so the reference could repair that stream where this library
    refuses it; for the other two it accepts none."""
    import carbonado_amd as ca
    from carbonado_amd.error import CarbonadoError
    spc = 3
    enc, h, info = _clean(spc, "header")
    memo = P.bao_prime(enc, h)
    (n,) = struct.unpack("<Q", enc[:8])
    assert n == 8192 * spc and n >> 13 & 1  # flipping bit 13 shrinks n
    streams = [struct.pack("<Q", n ^ 1 << bit) + enc[8:] for bit in (0, 40, 13)]
    oracle = [sorted(P.authentic_shards(bad, h, spc, memo)) for bad in streams]
    import torch
    from carbonado_amd import device as D
    count, L = len(streams), len(enc)
    stride = (off + L + 15) // 16 * 16 + 16
    host = np.full((count, stride), SENT, dtype=np.uint8)
    for o, bad in enumerate(streams):
        host[o, off:off + L] = np.frombuffer(bad, dtype=np.uint8)
    hashes = torch.from_numpy(np.frombuffer(h * count, dtype=np.uint8).reshape(count, 32).copy()).cuda()
    out = torch.full((count, stride), SENT, dtype=torch.uint8, device="cuda")
    status = D.scrub_batch(torch.from_numpy(host).cuda(), L, hashes, info.padding_len, info.chunk_len, out,
                           D.scrub_scratch(L, count), offset=off)
    torch.cuda.synchronize()
    single = []
    for bad in streams:
        try:
            ca.scrub(bad, h, info)
            single.append((0, ""))
        except CarbonadoError as e:
            single.append((e.status, getattr(e, "kind", "")))
    print("header damage codes: batch", status.tolist(), "single", single, "oracle's authentic shards", oracle)
    assert all(s != 0 for s in status.tolist()) and all(s != 0 for s, _ in single)
    assert (out.cpu().numpy() == SENT).all()


# ---- f. verify_slice on damaged level-4 streams ------------------------------

def _slice_grid(N):
    return [(0, 0), (N // 2, 0), (N - 1, 0), (0, 1), (N - 1, 1), (N + 2, 1), (0, N), (N // 2, 2), (1, N)]


def _verify_both(enc_bad, h, n, memo, tag):
    """ca.verify_slice == the oracle's bytes, or raises exactly when it raises."""
    import carbonado_amd as ca
    from carbonado_amd.error import BaoDecodeError
    N = max(1, -(-n // 1024))
    raised = 0
    for index, count in _slice_grid(N):
        start, length = index * 1024, count * 1024
        try:
            want = P.bao_decode_slice(P.bao_slice(enc_bad, start, length), h, start, length, memo)
        except P.SliceError:
            want = None
        try:
            got = ca.verify_slice(h, enc_bad, index, count)
        except BaoDecodeError:
            got = None
        assert got == want, (n, tag, index, count, "oracle raises" if want is None else "oracle accepts")
        raised += want is None
    return raised


@pytest.mark.parametrize("n", [1, 1023, 1025, 2049, 3000, 5121, 66561, 70001])
def test_verify_slice_damaged_level4(gpu, n):
    """Level-4 streams with a partial last chunk and odd promotions, every
    node damaged in turn (n <= 5121; above: the root, the ends of every level,
    parents over an eighth's boundary, the eighths' edge chunks), over a grid
    of (index, count): the oracle's bytes, or BaoDecodeError exactly when the
    oracle raises."""
    d = random.Random(n).randbytes(n)
    enc, h = O.bao_encode(d)
    memo = P.bao_prime(enc, h)
    nodes = B.tree_nodes(n)
    N = max(1, -(-n // 1024))
    assert len(nodes) == 2 * N - 1
    assert _verify_both(enc, h, n, memo, "clean") == 0
    if n <= 5121:
        cases = B.every_node_cases(nodes)
        assert len(cases) == 2 * (N - 1) + N
    else:
        cases = B.chosen_node_cases(nodes, N // 8)
        assert len(cases) >= 16 + 2 * (N - 1).bit_length()
    rng = random.Random(n + 1)
    for case in cases:
        raised = _verify_both(B.flip(enc, nodes, case, rng), h, n, memo, case)
        assert raised >= 2  # (0, N) and (1, N) walk every node but chunk 0


@pytest.mark.parametrize("n", [0, 1])
def test_verify_slice_damaged_hash(gpu, n):
    import carbonado_amd as ca
    from carbonado_amd.error import BaoDecodeError
    d = b"\x5a" * n
    enc, h = O.bao_encode(d)
    assert ca.verify_slice(h, enc, 0, 1) == d == P.bao_decode_slice(P.bao_slice(enc, 0, 1024), h, 0, 1024)
    for bit in (0, 100, 255):
        bad = bytearray(h)
        bad[bit // 8] ^= 1 << bit % 8
        for index, count in [(0, 0), (0, 1), (3, 1)]:
            with pytest.raises(P.SliceError):
                P.bao_decode_slice(P.bao_slice(enc, index * 1024, count * 1024), bytes(bad), index * 1024, count * 1024)
            with pytest.raises(BaoDecodeError):
                ca.verify_slice(bytes(bad), enc, index, count)
