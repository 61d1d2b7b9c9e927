"""The device-planned plaintext reads of level-13 streams
(include/carbonado_hip_kread.h) against the host-planned ones: for every
request set, content, content length, status, used and vouch of
read_plain_ranges_planned equal read_plain_ranges of the same requests placed at
r * stride, with the same keys, key status and flags.  What the host-planned
call refuses for a whole call (a stream index past the table, a start above
2^53 - 97, a len above 2^53, a range that ends above 2^36 - 32) and what it has
no word for (content longer than the capacity) is status 1 per request here;
the reference reads an empty range in that request's place.

Streams are level-13 encodings made on the device (encode_ragged_ecies, injected
ephemeral secrets and nonces) whose envelopes have 98, 1097, 4096 (no padding),
8097, 16384 and 262044 bytes (shard lengths 1024 to 65536), one described with a
chunk_len that does not fit (7), one whose key_status is 17 (killed), one read
under a wrong key (status 0, the host call's same wrong bytes), and damaged
ones: a flipped bit in a primary chunk (rebuilt and vouched), five shards
damaged (7), a damaged parent above a rebuilt chunk (unvouched; 5 under
CHIPV_STRICT).  All damage is flipped data bytes in streams.  The content buffer
is filled with a canary and only [0, content_len[r]) of a slot may change; the
scratch carries guard bytes behind the length the call is told."""
import functools

import numpy as np
import pytest

import read_world as RW  # tests/read_world.py (tests/ is on sys.path under pytest)
from bao_damage import chunk_off
from read_world import CANARY, Got, assert_equal

pytestmark = pytest.mark.gpu

SECRET = bytes(range(1, 33))
# envelopes: 0..5 intact; then misfit, killed, wrong key, and three damaged ones (8 chunks each: chunk i = shard i)
ENVS = [98, 1097, 4096, 8097, 16384, 262044, 4096, 8097, 4096, 4096, 4096, 4096]
MISFIT, KILLED, WRONG, FLIPPED, FIVE, PARENT = 6, 7, 8, 9, 10, 11
SIZES = [n - 97 for n in ENVS]  # plaintext bytes
SHARD = [1024, 1024, 1024, 2048, 4096, 65536, 1024, 2048, 1024, 1024, 1024, 1024]
REFUSED, KILL_STATUS, STRICT = 1, 17, 1
SPAN = 127 * 16  # bytes of one wave's span


class World:
    """The resident streams, their two tables and their keys, made once."""

    def __init__(self):
        import torch
        from carbonado_amd import device as D
        from oracle import oracle as O
        self.torch, self.D = torch, D
        count = len(SIZES)
        rng = np.random.default_rng(23)
        pitch = 1 << 18
        self.pt = [rng.integers(0, 256, n, dtype=np.uint8) for n in SIZES]
        plain = np.full(count * pitch, 0x11, dtype=np.uint8)
        for o, p in enumerate(self.pt):
            plain[o * pitch:o * pitch + p.size] = p
        in_off = [o * pitch for o in range(count)]
        inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
                  for _ in SIZES]
        self.off, _, total = D.ragged_layout(12, ENVS, 256)
        self.buf = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        self.len, infos = D.encode_ragged_ecies(13, O.c_public_key(SECRET), torch.from_numpy(plain).cuda(), in_off, SIZES,
                                                self.buf, self.off, self.hashes, D.ecies_ragged_scratch(13, SIZES),
                                                inject=inject)
        torch.cuda.synchronize()
        self.pads = [i.padding_len for i in infos]
        self.cls = [i.chunk_len for i in infos]
        assert self.cls == SHARD and self.pads[2] == 0 and self.pads[0] == 4096 - 98 and self.pads[5] == 100
        # the keys of the intact streams as they are described truly
        keys, ivs, kstat = D.stream_keys(SECRET, self.buf, self.off, self.len, self.hashes, self.pads, self.cls,
                                         D.stream_keys_scratch(count))
        assert not kstat.any()
        self.keys, self.ivs, self.kstat = keys.copy(), ivs.copy(), kstat.copy()
        self.kstat[KILLED] = KILL_STATUS
        self.keys[WRONG] = np.roll(self.keys[WRONG], 1) ^ 0x35
        self.cls[MISFIT] = 2048
        flips = [(FLIPPED, chunk_off(1, 8) + 300), (PARENT, chunk_off(2, 8) - 64 + 5)]  # the CV of chunk 2 in its parent
        flips += [(FIVE, chunk_off(i, 8) + 40 + i) for i in (1, 0, 4, 6, 2)]
        at = torch.tensor([self.off[s] + o for s, o in flips], dtype=torch.int64, device="cuda")
        self.buf[at] ^= 0x10
        torch.cuda.synchronize()
        self.host = self.buf.cpu().numpy().copy()
        self.table = D.stream_table(self.buf, self.off, self.len, self.hashes, self.pads, self.cls)
        self.ktab = D.key_table(self.keys, self.ivs, self.kstat)
        torch.cuda.synchronize()
        assert (self.table.nstreams, self.table.max_chunks, self.table.min_shard) == (count, 512, 1024)
        self.ktab_image = self.ktab.table.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def world() -> World:
    return World()


def base_requests(max_len):
    """[(stream, start, len, refused)] in plaintext bytes"""
    P5 = SIZES[5]
    out = [(2, 100, 200, 0)]                                             # inside one chunk
    out += [(5, 1000 + k, 300 + k, 0) for k in range(16)]                # every start residue mod 16
    for ln in (0, 1, 15, 16, 17, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN, max_len):
        out += [(5, 70000 + 5, ln, 0), (5, 80000, ln, 0)]                # the span's edges, start residue 5 and 0
    out += [(5, 90000 + 15, SPAN, 0), (4, 1, SPAN + 16, 0)]              # lane 63 without a neighbour; into the next span
    out += [(3, 1024 - 97 - 10, 100, 0), (5, 2 * 65536 - 97 - 6, 10, 0), (4, 4096 - 97 - 6, 12, 0)]  # chunk / shard boundary
    out += [(2, 1024 - 97 - 50, 1100, 0), (2, 0, 3999, 0), (2, 927, 3072, 0)]  # 2 and 4 shards
    out += [(2, 5, 0, 0), (1, 1000, 10, 0), (1, 5000, 1, 0), (0, 1, 1, 0)]  # len 0, start >= P
    out += [(1, 990, 100, 0), (0, 0, 50, 0), (5, P5 - 50, 4096, 0), (3, 7990, max_len, 0)]  # clipped at P
    out += [(5, 65536 - 2000, max_len, 0), (4, 4096 * 2 - 7, max_len, 0), (3, 3, max_len, 0)]  # the whole capacity
    out += [(4, 0, max_len + 1, REFUSED), (5, 17, 1 << 40, REFUSED)]     # content longer than max_len
    out += [(len(SIZES), 0, 10, REFUSED), (2, (1 << 53) - 96, 10, REFUSED), (2, 0, (1 << 53) + 1, REFUSED)]
    out += [(5, (1 << 36) - 31, 10, REFUSED), (2, (1 << 53) - 97, 0, REFUSED)]  # ends above 2^36 - 32
    out += [(5, (1 << 36) - 32, 10, 0)]                                  # at the limit: empty, not refused
    out += [(MISFIT, 0, 100, 0)]                                         # chunk_len does not fit: 7
    out += [(KILLED, 100, 200, 0), (KILLED, 0, 0, 0), (KILLED, 7990, 100, 0), (KILLED, 9000, 5, 0),
            (KILLED, 3, max_len, 0), (KILLED, 0, max_len + 1, REFUSED)]  # killed; refused comes first
    out += [(WRONG, 10, 500, 0), (WRONG, 0, 3999, 0)]
    out += [(FLIPPED, 1027, 200, 0), (FLIPPED, 903, 1500, 0), (FLIPPED, 1951, 100, 0)]
    out += [(FIVE, 937, 50, 0), (FIVE, 2975, 20, 0)]
    out += [(PARENT, 1961, 100, 0), (PARENT, 0, 3999, 0)]
    return out


class Planned(RW.Planned):
    def scratch_len(self):
        return self.w.D.planned_plain_read_scratch(self.table, self.nreq, self.max_len).numel()

    def enqueue(self, flags=0):
        self.w.D.read_plain_ranges_planned(self.table, self.w.ktab, self.rs, self.start, self.length, self.max_len,
                                           self.content, self.stride, self.clen, self.status, self.used, self.vouch,
                                           self.scratch, flags)


@functools.lru_cache(maxsize=None)
def _reference(reqs, stride, flags) -> Got:
    w = world()
    torch, D = w.torch, w.D
    n = len(reqs)
    rs, start, length, coff = RW.host_requests(reqs, stride)
    _, _, _, nseg = D.plain_read_layout(w.cls, w.pads, rs, start, length)
    content = torch.full((n * stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
    status, used, vouch = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    clen = D.read_plain_ranges(w.keys, w.ivs, w.kstat, w.buf, w.off, w.len, w.hashes, w.pads, w.cls, rs, start, length,
                               content, coff, status, used, vouch, D.plain_read_scratch(n, nseg, len(SIZES)), flags=flags)
    return RW.host_result(reqs, clen, content, status, used, vouch)


def reference(w: World, reqs, max_len, stride, flags=0) -> Got:
    """The host-planned call over the same requests at r * stride (computed once
    per request set); a refused request reads an empty range there and has
    status 1, used 0, vouch 0 here."""
    return _reference(tuple(reqs), stride, flags)


def _requests(nreq, max_len):
    base = base_requests(max_len)
    return [base[(r + 50) % len(base)] for r in range(nreq)]


def test_base_set_is_what_it_says(gpu):
    """The reference itself: the test's own plaintexts, and every class of stream is there."""
    w = world()
    for max_len in (4096, 5000):
        reqs = base_requests(max_len)
        stride = (max_len + 15) // 16 * 16 + 16
        ref = reference(w, reqs, max_len, stride)
        by = {rq[:3]: r for r, rq in enumerate(reqs)}
        assert {rq[1] % 16 for rq in reqs if rq[0] == 5 and rq[2] and not rq[3]} == set(range(16))
        for r, (s, start, ln, refused) in enumerate(reqs):
            if refused or s in (MISFIT, KILLED, WRONG, FIVE):
                continue
            want = w.pt[s][start:start + ln]
            assert ref.clen[r] == len(want) and ref.status[r] == 0, reqs[r]
            assert np.array_equal(ref.content[r * stride:r * stride + len(want)], want), reqs[r]
        assert ref.clen[by[2, 0, 3999]] == 3999 and ref.used[by[2, 0, 3999]] == 0b1111
        assert ref.status[by[MISFIT, 0, 100]] == 7
        for rq, n in (((KILLED, 100, 200), 200), ((KILLED, 0, 0), 0), ((KILLED, 7990, 100), 10), ((KILLED, 9000, 5), 0),
                      ((KILLED, 3, max_len), max_len)):
            r = by[rq]
            assert (ref.status[r], ref.used[r], ref.vouch[r], ref.clen[r]) == (KILL_STATUS, 0, 0, n)
            assert not ref.content[r * stride:r * stride + n].any()
        r = by[WRONG, 10, 500]
        assert ref.status[r] == 0 and ref.clen[r] == 500
        assert not np.array_equal(ref.content[r * stride:r * stride + 500], w.pt[WRONG][10:510])
        r = by[FLIPPED, 1027, 200]
        assert (ref.status[r], ref.used[r], ref.vouch[r]) == (0, 0b11101, 1)            # rebuilt and vouched
        assert ref.used[by[FLIPPED, 1951, 100]] == 0b100                                # not the damaged primary
        assert ref.status[by[FIVE, 937, 50]] == 7 and ref.status[by[FIVE, 2975, 20]] == 0
        r = by[PARENT, 1961, 100]
        assert (ref.status[r], ref.vouch[r]) == (0, 2)                                  # unvouched
        strict = reference(w, reqs, max_len, stride, STRICT)
        assert strict.status[r] != 0 and not strict.content[r * stride:r * stride + 100].any()
        assert ref.clen[by[5, (1 << 36) - 32, 10]] == 0 and ref.status[by[5, (1 << 36) - 32, 10]] == 0


def test_key_table_holds_what_the_header_says(gpu):
    from carbonado_amd import _lib
    w = world()
    n = len(SIZES)
    img = w.ktab_image
    words = 512 * n
    raw = words + (4 * n + 15) // 16 * 16
    assert img.size == raw + 48 * n == _lib.lib().chipk_key_table_len(n)
    assert np.array_equal(img[words:words + 4 * n].view(np.uint32), w.kstat)
    assert not img[raw:].any(), "the raw keys stayed in the table"
    recs = img[:words].reshape(n, 512)
    assert not recs[KILLED].any() and all(recs[s].any() for s in range(n) if s != KILLED)
    assert not recs[:, 496:].any()                              # the padding of a record
    assert not np.array_equal(recs[2], recs[WRONG])


@pytest.mark.parametrize("max_len", [4096, 5000])
@pytest.mark.parametrize("nreq", [1, 63, 64, 65, 257])
def test_planned_equals_host_planned(gpu, nreq, max_len):
    w = world()
    reqs = _requests(nreq, max_len)
    assert nreq < 63 or (sum(r[3] for r in reqs) >= 5 and sum(r[0] == KILLED for r in reqs) >= 5)
    p = Planned(w, nreq, max_len)
    for flags in (0, STRICT):
        got = p.run(reqs, flags)
        assert_equal(got, reference(w, reqs, max_len, p.stride, flags), reqs)
        for r, (s, start, ln, refused) in enumerate(reqs):      # and the test's own plaintexts
            if not refused and s <= 5:
                want = w.pt[s][start:start + ln]
                assert got.status[r] == 0 and np.array_equal(got.content[r * p.stride:r * p.stride + len(want)], want)
    assert np.array_equal(w.buf.cpu().numpy(), w.host), "a read changed the streams"
    assert np.array_equal(w.ktab.table.cpu().numpy(), w.ktab_image), "a read changed the key table"


def test_every_request_alone(gpu):
    """Capacity 1, each request of the base set in turn: the result it has inside the batch."""
    w = world()
    base = base_requests(4096)
    p = Planned(w, 1, 4096)
    batch = reference(w, base, 4096, p.stride)
    for r, rq in enumerate(base):
        got = p.run([rq])
        assert_equal(got, reference(w, [rq], 4096, p.stride), [rq])
        assert (got.status[0], got.used[0], got.vouch[0], got.clen[0]) == (batch.status[r], batch.used[r], batch.vouch[r],
                                                                          batch.clen[r]), rq
        assert np.array_equal(got.content[:p.stride], batch.content[r * p.stride:(r + 1) * p.stride]), rq


def test_lying_info_refuses_that_streams_requests(gpu):
    w = world()
    from carbonado_amd import _lib
    info = _lib.TableInfo(w.table.info.nstreams, w.table.info.max_chunks - 1, w.table.info.min_shard, 0)
    lying = w.D.StreamTable(w.table.table, info)
    reqs = _requests(64, 4096)
    assert any(r[0] == 5 and not r[3] for r in reqs)
    got = Planned(w, 64, 4096, table=lying).run(reqs)
    # stream 5 alone has 512 chunks: its requests are refused, every other request is as before
    marked = [(s, a, b, REFUSED if s == 5 else f) for s, a, b, f in reqs]
    assert_equal(got, reference(w, marked, 4096, (4096 + 15) // 16 * 16 + 16), marked)


def test_graph_replay_with_requests_rewritten_in_place(gpu):
    w = world()
    torch = w.torch
    nreq, max_len = 65, 4096
    p = Planned(w, nreq, max_len)
    side = torch.cuda.Stream()
    p.set(_requests(nreq, max_len))
    with torch.cuda.stream(side):
        p.enqueue()  # the warm-up: the thread's context exists from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        p.enqueue()
    base = base_requests(max_len)
    for k in range(3):
        reqs = [base[(7 * k + 3 * r + 1) % len(base)] for r in range(nreq)]
        assert any(r[3] for r in reqs) and any(r[0] == KILLED and not r[3] for r in reqs)
        p.set(reqs)
        p.clen.fill_(-1); p.status[:nreq].fill_(-1); p.used[:nreq].fill_(-1); p.vouch[:nreq].fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        assert_equal(p.result(), reference(w, reqs, max_len, p.stride), reqs)
    assert np.array_equal(w.ktab.table.cpu().numpy(), w.ktab_image)


def test_wipe_leaves_zeros(gpu):
    """A table of its own (the world's serves the other tests): zeros over all of it."""
    w = world()
    tab = w.D.key_table(w.keys, w.ivs, w.kstat)
    w.torch.cuda.synchronize()
    assert np.array_equal(tab.table.cpu().numpy(), w.ktab_image)   # the setup is a function of its arguments
    w.D.wipe_key_table(tab)
    w.torch.cuda.synchronize()
    assert not tab.table.cpu().numpy().any()
    # key_status None: every stream has a record
    tab = w.D.key_table(w.keys, w.ivs, None)
    w.torch.cuda.synchronize()
    img = tab.table.cpu().numpy()
    assert img[:512 * len(SIZES)].reshape(len(SIZES), 512)[KILLED].any() and not img[512 * len(SIZES):].any()
    w.D.wipe_key_table(tab)
