"""read_ranges (include/carbonado_hip_read.h) against the independent slice
verifier: byte ranges of level-12 streams of seven sizes with damaged chunks,
parents, roots and headers in ONE call.  Whether slice (segment, shard) may be
trusted comes from oracle/pyoracle.py (bao_decode_slice over bao_slice of the
damaged stream, the same chunk window of every shard); status, `used` and the
content follow from those verdicts by the header's rule and are exact: own
slice good -> copied, bit p; else the four lowest good shards -> rebuilt, their
bits; fewer than four -> 7, zeros.  Authentic content is the original object's
bytes.  The content buffer is filled with a sentinel and only the requests'
ranges may change; the input must not change; the scratch carries guard bytes
past the length the call is told.  Streams sit at offsets 56 and 8 mod 256."""
import functools
import random
from typing import NamedTuple

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
import test_gpu_scrub_ragged as SR
from oracle import oracle as O
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SENT, GUARD = SR.SENT, SR.GUARD
# one chunk per shard, odd trees, the first two-group tree (9), shards over several 64-chunk subtrees (33)
SPCS = [1, 2, 3, 5, 8, 9, 33]
DAMAGES = ("none", "chunk", "level-1 parent", "root", "header", "four shards", "five shards")


class Stream(NamedTuple):
    spc: int
    data: bytes      # the object
    clean: bytes     # O.encode's stream
    flips: tuple     # (stream offset, xor mask) of every damaged bit
    hash: bytes
    padding: int
    chunk_len: int
    what: str
    memo: dict

    @property
    def bad(self) -> bytes:
        return B.apply(self.clean, self.flips)


class Req(NamedTuple):
    stream: int
    start: int
    len: int


class Want(NamedTuple):
    status: int
    used: int
    content: bytes   # what the range must hold (zeros for a failed request)


def _stream(spc: int, seed, what: str, damage) -> Stream:
    """`damage(nodes, chunks, rng)` -> what to flip one bit in: (node number,
    half) cases of tests/bao_damage.py, or ("raw", stream offset, xor mask)."""
    enc, h, pad, cl = SR._clean(spc, seed)
    data = random.Random(repr(seed)).randbytes(4096 * spc - 37 - spc)  # what _clean encoded
    nodes = B.tree_nodes(8192 * spc)
    chunks = [k for k, nd in enumerate(nodes) if not nd.parent]
    assert b"".join(enc[nodes[k].off:nodes[k].off + 1024] for k in chunks[:4 * spc])[:len(data)] == data
    rng = random.Random(f"read{seed}")
    flips = tuple(x[1:] if x[0] == "raw" else B.pick(nodes, x, rng) for x in damage(nodes, chunks, rng))
    return Stream(spc, data, enc, flips, h, pad, cl, what, P.bao_prime(enc, h, {}))


def _focus(spc: int) -> int:
    """The chunk of a shard the sized streams are damaged in."""
    return spc // 2


def _sized_stream(spc: int, what: str) -> Stream:
    j = _focus(spc)

    def damage(nodes, chunks, rng):
        if what == "none":
            return []
        if what == "chunk":
            return [(chunks[spc + j], -1)]
        if what == "level-1 parent":
            (k,) = [k for k, nd in enumerate(nodes) if nd.level == 1 and nd.lo <= spc + j < nd.hi]
            return [(k, rng.randrange(2))]
        if what == "root":
            return [(0, rng.randrange(2))]
        if what == "header":
            return [("raw", rng.randrange(8), 1 << rng.randrange(8))]
        shards = (1, 0, 4, 6) if what == "four shards" else (1, 0, 4, 6, 2)
        return [(chunks[i * spc + j], -1) for i in shards]
    return _stream(spc, (what, spc), what, damage)


def _ranges(st: Stream):
    """The ranges every sized stream is read at (start, len), in object bytes."""
    C, spc, j = st.chunk_len, st.spc, _focus(st.spc)
    n_obj = 4 * C - st.padding
    at = C + 1024 * j                      # object byte of the focus chunk of primary 1
    out = [(0, 1), (n_obj - 1, 1),
           (at + 133, 300),                # inside the focus chunk, start % 16 != 0
           (at - 5, 10), (at - 5, 40),     # across a chunk boundary (spc 1: the primary boundary)
           (at + 1024 - 5, 10), (1024 - 5, 40),
           (C - 5, 10), (3 * C - 5, 10),   # across a primary boundary
           (0, n_obj), (0, 4 * C + 100),   # the whole object: four segments
           (n_obj - 50, 200),              # ending inside the padding: clipped
           (n_obj, 10), (4 * C + 5, 1), (17, 0),  # empty
           (3 * C + 11, 500)]
    if spc >= 2:                           # primary 1, but not the focus chunk: its damage is outside the window
        out.append((C + 1024 * ((j + 1) % spc) + 7, 100))
    return out


@functools.lru_cache(maxsize=None)
def main_set():
    """(streams, requests): per size every damage with every range; for spc = 2
    all 256 sets of damaged shards (chunk 0 of each) with a one-chunk window and
    a two-chunk window in each primary."""
    streams, reqs = [], []
    for spc in SPCS:
        for what in DAMAGES:
            st = _sized_stream(spc, what)
            reqs += [Req(len(streams), a, b) for a, b in _ranges(st)]
            streams.append(st)
    spc = 2
    for m in range(256):
        st = _stream(spc, ("rmask", m), f"damaged {m:#04x}",
                     lambda nodes, chunks, rng, m=m: [(chunks[i * spc], -1) for i in range(8) if m >> i & 1])
        for p in range(4):
            reqs += [Req(len(streams), p * st.chunk_len + 100, 200), Req(len(streams), p * st.chunk_len + 1000, 100)]
        streams.append(st)
    return tuple(streams), tuple(reqs)


def _segments(st: Stream, start: int, length: int):
    """[(p, c0, c1)] of a request, by plain arithmetic."""
    C = st.chunk_len
    n_obj = 4 * C - st.padding
    end = min(n_obj, start + length)
    if length == 0 or start >= n_obj:
        return []
    return [(p, max(start, p * C) - p * C, min(end, (p + 1) * C) - p * C) for p in range(start // C, (end - 1) // C + 1)]


def _verdict(st: Stream, bad: bytes, cache: dict, i: int, w0: int, w1: int) -> bool:
    key = (i, w0, w1)
    if key not in cache:
        start, ln = (i * st.spc + w0) * 1024, (w1 - w0) * 1024
        try:
            P.bao_decode_slice(P.bao_slice(bad, start, ln), st.hash, start, ln, st.memo)
            cache[key] = True
        except P.SliceError:
            cache[key] = False
    return cache[key]


def expected(streams, reqs, overrides=None):
    """Want per request, from the independent verifier's verdicts."""
    bads = [(overrides or {}).get(s, st.bad) for s, st in enumerate(streams)]
    caches = [{} for _ in streams]
    out = []
    for rq in reqs:
        st = streams[rq.stream]
        segs = _segments(st, rq.start, rq.len)
        size = sum(c1 - c0 for _, c0, c1 in segs)
        used, ok = 0, True
        for p, c0, c1 in segs:
            w0, w1 = c0 // 1024, -(-c1 // 1024)
            v = functools.partial(_verdict, st, bads[rq.stream], caches[rq.stream], w0=w0, w1=w1)
            if v(p):
                used |= 1 << p
                continue
            good = [i for i in range(8) if i != p and v(i)]
            if len(good) < 4:
                ok = False
                break
            used |= sum(1 << i for i in good[:4])
        out.append(Want(0, used, st.data[rq.start:rq.start + size]) if ok else Want(7, 0, bytes(size)))
    return out


@functools.lru_cache(maxsize=None)
def main_expected():
    return tuple(expected(*main_set()))


class Result(NamedTuple):
    status: np.ndarray
    used: np.ndarray
    content: np.ndarray  # the whole content buffer afterwards
    off: list
    clen: list


def _place(streams):
    off, cur = [], 0
    for j, st in enumerate(streams):
        off.append(cur + (56 if j % 2 == 0 else 8))
        cur = -(-(off[-1] + len(st.clean) + 24) // 256) * 256
    return off, cur


class Call:
    """The device side of one set: buffers made once, read() as often as wanted."""

    def __init__(self, streams, reqs, align=16, overrides=None, chunk_len=None, padding=None):
        import torch
        from carbonado_amd import device as D
        self.D, self.torch = D, torch
        self.streams, self.reqs = streams, reqs
        self.in_off, total = _place(streams)
        self.host = np.full(total, SENT, dtype=np.uint8)
        for s, st in enumerate(streams):
            b = (overrides or {}).get(s, st.bad)
            self.host[self.in_off[s]:self.in_off[s] + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.inp = torch.from_numpy(self.host).cuda()
        self.in_len = [len(st.clean) for st in streams]
        self.pads = [(padding or {}).get(s, st.padding) for s, st in enumerate(streams)]
        self.cls = [(chunk_len or {}).get(s, st.chunk_len) for s, st in enumerate(streams)]
        self.hashes = SR._hashes(streams)
        self.rs, self.start, self.len = [r.stream for r in reqs], [r.start for r in reqs], [r.len for r in reqs]
        self.off, self.clen, self.total, self.nseg = D.read_layout(self.cls, self.pads, self.rs, self.start, self.len, align)
        need = D.read_scratch(len(reqs), self.nseg).numel()
        self.full = torch.full((need + 256,), GUARD, dtype=torch.uint8, device="cuda")
        self.scratch = self.full[:need]
        self.content = torch.full((self.total + 64,), SENT, dtype=torch.uint8, device="cuda")
        self.status = torch.full((len(reqs) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.used = torch.full((len(reqs) + 8,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")

    def read(self) -> Result:
        torch, n = self.torch, len(self.reqs)
        clen = self.D.read_ranges(self.inp, self.in_off, self.in_len, self.hashes, self.pads, self.cls, self.rs, self.start,
                                  self.len, self.content, self.off, self.status, self.used, self.scratch)
        torch.cuda.synchronize()
        assert (self.full[self.scratch.numel():] == GUARD).all().item(), "bytes past scratch_len were written"
        assert np.array_equal(self.inp.cpu().numpy(), self.host), "read_ranges changed its input"
        assert (self.status[n:] == 0x5A5A5A5A).all().item() and (self.used[n:] == 0x3C3C3C3C).all().item()
        return Result(self.status[:n].cpu().numpy(), self.used[:n].cpu().numpy(), self.content.cpu().numpy(), self.off,
                      clen)


def _check(call: Call, res: Result, want):
    reqs, streams = call.reqs, call.streams

    def who(r):
        st = streams[reqs[r].stream]
        return (r, st.spc, st.what, reqs[r].start, reqs[r].len)
    assert res.clen == [len(w.content) for w in want]
    bad = [(who(r), int(res.status[r]), w.status) for r, w in enumerate(want) if res.status[r] != w.status]
    assert not bad, bad[:8]
    bad = [(who(r), hex(int(res.used[r])), hex(w.used)) for r, w in enumerate(want) if res.used[r] != w.used]
    assert not bad, bad[:8]
    expect = np.full(res.content.size, SENT, dtype=np.uint8)  # sentinels between and behind the ranges
    for r, w in enumerate(want):
        expect[res.off[r]:res.off[r] + len(w.content)] = np.frombuffer(w.content, dtype=np.uint8)
    if not np.array_equal(res.content, expect):
        at = int(np.flatnonzero(res.content != expect)[0])
        r = max(k for k in range(len(reqs)) if res.off[k] <= at)
        raise AssertionError(f"content differs at byte {at}: request {who(r)} status {want[r].status} used "
                             f"{want[r].used:#x}, {at - res.off[r]} bytes into its range of {len(want[r].content)}")


@functools.lru_cache(maxsize=None)
def main_call() -> Call:
    return Call(*main_set())


@functools.lru_cache(maxsize=None)
def main_result() -> Result:
    return main_call().read()


def test_every_size_range_and_damage_in_one_call(gpu):
    streams, reqs = main_set()
    want = main_expected()
    assert len(streams) == len(SPCS) * len(DAMAGES) + 256 and len(reqs) > 2500
    assert {x % 256 for x in main_call().in_off} == {56, 8}
    # nothing vacuous: the verdicts are the ones the damage was built for
    by = {(st.spc, st.what): s for s, st in enumerate(streams)}
    pick = {(st, a): want[r] for r, (st, a, _) in enumerate(reqs)}
    for spc in SPCS:
        C, j = 1024 * spc, _focus(spc)
        focus = C + 1024 * j + 133
        assert pick[by[spc, "none"], focus].used == 0b10 and pick[by[spc, "chunk"], focus].used == 0b11101
        assert pick[by[spc, "level-1 parent"], focus].status == 0 and pick[by[spc, "level-1 parent"], focus].used & 2 == 0
        assert pick[by[spc, "four shards"], focus].used == 0b10101100 and pick[by[spc, "five shards"], focus].status == 7
        assert all(w.status == 7 for r, w in enumerate(want)
                   if streams[reqs[r].stream].what in ("root", "header") and streams[reqs[r].stream].spc == spc
                   and w.content)
        assert pick[by[spc, "chunk"], 3 * C + 11].used == 0b1000           # another primary: direct
        if spc >= 2:
            assert pick[by[spc, "chunk"], C + 1024 * ((j + 1) % spc) + 7].used == 0b10  # damage outside the window
        whole = [want[r] for r, q in enumerate(reqs) if q.stream == by[spc, "chunk"] and q.start == 0 and q.len > 1]
        assert len(whole) == 2 and all(w.used == 0b11101 and len(w.content) == 4 * C - 37 - spc for w in whole)
    masks = [(int(streams[q.stream].what.split()[1], 16), q.start // 2048, w) for q, w in zip(reqs, want)
             if streams[q.stream].what.startswith("damaged")]
    assert len(masks) == 2048
    for m, p, w in masks:
        good = [i for i in range(8) if not m >> i & 1]
        if not m >> p & 1:
            assert (w.status, w.used) == (0, 1 << p)
        elif len(good) >= 4:
            assert (w.status, w.used) == (0, sum(1 << i for i in good[:4]))
        else:
            assert (w.status, w.used) == (7, 0)
    assert {w.status for w in want} == {0, 7} and len({w.used for w in want}) >= 70
    assert main_call().clen == [len(w.content) for w in want]  # the layout call's lengths
    _check(main_call(), main_result(), want)


def test_repeat_over_the_same_buffers(gpu):
    """The same call again: same scratch (now holding the first call's words),
    status and used pre-filled with garbage, the content with another sentinel
    pattern left from the first call: every word and byte is set again."""
    call, first = main_call(), main_result()
    n = len(call.reqs)
    call.status[:n] = 0x7F7F7F7F
    call.used[:n] = -1
    for r, w in enumerate(main_expected()):
        if w.content:
            call.content[call.off[r]:call.off[r] + len(w.content)] = 0xEE
    again = call.read()
    _check(call, again, main_expected())
    assert np.array_equal(again.status, first.status) and np.array_equal(again.used, first.used)


def test_content_offsets_at_align_256(gpu):
    streams, reqs = main_set()
    keep = [r for r, q in enumerate(reqs) if not streams[q.stream].what.startswith("damaged")]
    call = Call(streams, tuple(reqs[r] for r in keep), align=256)
    assert all(x % 256 == 0 for x in call.off) and len(set(call.off)) > len(keep) // 2
    _check(call, call.read(), [main_expected()[r] for r in keep])


def test_per_stream_errors_leave_the_neighbours_alone(gpu):
    """A chunk_len that does not fit and a padding above four shards are that
    request's status 7 with no content; the other requests are as before."""
    streams, reqs = main_set()
    pick = [s for s, st in enumerate(streams) if st.spc in (3, 9) and st.what in ("none", "chunk")]
    sub = tuple(streams[s] for s in pick)
    rq = tuple(Req(pick.index(q.stream), q.start, q.len) for q in reqs if q.stream in pick)
    base = [w for q, w in zip(reqs, main_expected()) if q.stream in pick]
    call = Call(sub, rq, chunk_len={0: sub[0].chunk_len + 1024, 1: 0}, padding={2: 4 * sub[2].chunk_len + 1})
    want = [Want(7, 0, b"") if q.stream < 3 else w for q, w in zip(rq, base)]
    assert any(w.content for w in want) and any(w.status == 7 and not w.content for w in want)
    _check(call, call.read(), want)


def test_intact_reads_agree_with_verify_slices(gpu):
    """Chunk-aligned ranges inside one primary of intact streams: the content of
    device.verify_slices over the same chunks."""
    import torch
    from carbonado_amd import device as D
    streams = tuple(st for st in main_set()[0] if st.what == "none")
    reqs, idx, cnt = [], [], []
    for s, st in enumerate(streams):
        for p, w0, n in ((0, 0, 1), (1, st.spc // 2, 1), (2, 0, st.spc), (3, 0, max(1, st.spc - 1))):
            reqs.append(Req(s, p * st.chunk_len + 1024 * w0, 1024 * n))
            idx.append(p * st.spc + w0)
            cnt.append(n)
    call = Call(streams, tuple(reqs))
    res = call.read()
    assert (res.status == 0).all() and [int(u) for u in res.used] == [1 << (q.start // streams[q.stream].chunk_len)
                                                                      for q in reqs]
    n8 = [8 * st.chunk_len for st in streams]
    _, _, coff, clen, _, ctotal = D.slice_layout([n8[q.stream] for q in reqs], idx, cnt)
    content = torch.zeros(ctotal, dtype=torch.uint8, device="cuda")
    status = torch.full((len(reqs),), -1, dtype=torch.int32, device="cuda")
    got = D.verify_slices(call.inp, call.in_off, call.in_len, call.hashes, call.rs, idx, cnt, content, coff, status,
                          D.audit_scratch(len(streams), len(reqs)))
    torch.cuda.synchronize()
    assert (status == 0).all().item() and got == clen
    theirs = content.cpu().numpy()
    for r in range(len(reqs)):
        mine = res.content[res.off[r]:res.off[r] + res.clen[r]]
        assert np.array_equal(mine, theirs[coff[r]:coff[r] + res.clen[r]]), r  # (the last primary: clipped at n_obj)
        assert res.clen[r] == min(clen[r], 4 * streams[reqs[r].stream].chunk_len - streams[reqs[r].stream].padding
                                  - reqs[r].start)


def test_damaged_reads_agree_with_scrub_then_decode(gpu):
    """Repairable streams: every served range equals the same bytes of
    decode_ragged run on scrub_ragged's output."""
    import torch
    from carbonado_amd import device as D
    streams, reqs = main_set()
    pick = [s for s, st in enumerate(streams) if st.what in ("chunk", "level-1 parent", "four shards")]
    pick += [s for s, st in enumerate(streams) if st.what.startswith("damaged")][5::16]
    sub = [streams[s] for s in pick]
    rq = tuple(Req(pick.index(q.stream), q.start, q.len) for q in reqs if q.stream in pick)
    call = Call(tuple(sub), rq)
    res = call.read()
    out = torch.full((call.inp.numel(),), SENT, dtype=torch.uint8, device="cuda")
    st = D.scrub_ragged(call.inp, call.in_off, call.in_len, call.hashes, call.pads, call.cls, out, call.in_off,
                        D.scrub_ragged_scratch(call.in_len))
    fixed = [s for s in range(len(sub)) if st[s] == 0]
    assert len(fixed) > len(sub) // 2
    ooff, cur = [], 0
    for s in fixed:
        ooff.append(cur)
        cur += -(-4 * sub[s].chunk_len // 256) * 256
    objs = torch.zeros(cur, dtype=torch.uint8, device="cuda")
    dstat = torch.full((len(fixed),), -1, dtype=torch.int32, device="cuda")
    lens = [call.in_len[s] for s in fixed]
    olen = D.decode_ragged(12, out, [call.in_off[s] for s in fixed], lens, call.hashes[fixed].contiguous(),
                           [call.pads[s] for s in fixed], objs, ooff, dstat, D.ragged_scratch(12, lens, decode=True))
    torch.cuda.synchronize()
    assert (dstat == 0).all().item()
    theirs = objs.cpu().numpy()
    seen = 0
    for r, q in enumerate(rq):
        if q.stream not in fixed or not res.clen[r]:
            continue
        k = fixed.index(q.stream)
        assert olen[k] == len(sub[q.stream].data)
        assert res.status[r] == 0
        mine = res.content[res.off[r]:res.off[r] + res.clen[r]]
        assert np.array_equal(mine, theirs[ooff[k] + q.start:ooff[k] + q.start + res.clen[r]]), (r, q)
        seen += int(res.used[r]) != 1 << (q.start // sub[q.stream].chunk_len)
    assert seen > 20  # rebuilt reads among them


def test_one_16_mib_object(gpu):
    """N = 32768 chunks: a 4 KiB read across a damaged chunk of primary 1 and
    the whole object, both rebuilt from shards 0, 2, 3, 4 where they must be."""
    spc = 4096
    d = np.random.default_rng(16).integers(0, 256, (16 << 20) - 41, dtype=np.uint8).tobytes()
    enc, h, info = O.encode(d, 12)
    assert info["chunk_len"] == 1024 * spc and info["padding_len"] == 41
    nodes = B.tree_nodes(8192 * spc)
    k = next(j for j, nd in enumerate(nodes) if not nd.parent and nd.lo == spc + 1234)
    flips = (B.pick(nodes, (k, -1), random.Random(16)),)
    st = Stream(spc, d, enc, flips, h, 41, 1024 * spc, "chunk 1234 of shard 1", P.bao_prime(enc, h, {}))
    C = 1024 * spc
    reqs = (Req(0, C + 1024 * 1234 - 1500, 4096), Req(0, 0, 4 * C), Req(0, C + 1024 * 1236 + 3, 4096))
    want = expected((st,), reqs)
    assert [(w.status, w.used) for w in want] == [(0, 0b11101), (0, 0b11101), (0, 0b10)]
    assert want[1].content == d and want[0].content == d[reqs[0].start:reqs[0].start + 4096]
    call = Call((st,), reqs)
    _check(call, call.read(), want)
