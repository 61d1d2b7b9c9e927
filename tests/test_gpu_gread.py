"""The device-planned plaintext reads of level-14 and level-15 streams
(include/carbonado_hip_gread.h) against the host-planned ones: for every
request set, content, content length, status, used and vouch of
read_frame_ranges_planned equal read_frame_ranges of the same requests placed at
r * stride, with the same streams, index, keys and flags, byte for byte and word
for word; there is no tolerance anywhere.  What the host-planned call refuses
for a whole call (a stream index past the table, a start or len above 2^53) and
what it has no word for (content longer than the capacity, a table that
contradicts its info) is status 1 per request here; the reference reads an
empty range in that request's place.  A stream killed by its key_status (15) is
a stream killed by its index_status with the same word in the reference, which
has no key_status.

The streams are the world of tests/test_gpu_fread.py: plaintexts of 0, 1,
65535, 65536, 65537, 131072, 131077 and 200003 bytes, random, compressible and
both inside one stream, at 14 and at 15.  The capacities 1, 4096, 65537 and
70000 bytes give fcap (the frames a range may touch) 1, 2, 2 and 3.  The
content buffer is filled with a canary and only [0, content_len[r]) of a slot
may change; the scratch carries guard bytes behind the length the call is
told."""
import functools

import numpy as np
import pytest

import read_world as RW  # tests/read_world.py (tests/ is on sys.path under pytest)
import test_gpu_fread as F
from read_world import CANARY, Got, assert_equal

pytestmark = pytest.mark.gpu

FRAME, SIZES, BIG, TWO_RAW, FORMATS = F.FRAME, F.SIZES, F.BIG, F.TWO_RAW, F.FORMATS
HASH, ZFEC, UNSUPPORTED, SNAP, VOUCHED = F.HASH, F.ZFEC, F.UNSUPPORTED, F.SNAP, F.VOUCHED
REFUSED, STRICT, KEY_KILL, UNVOUCHED = 1, 1, 17, 2
KILLED_11, KILLED_5, KEY_KILLED = 3, 6, 5   # streams of the "killed" variants


class Variant:
    """One state of the streams and their tables: what the planned call and the
    host-planned reference are both given."""

    def __init__(self, w, out=None, istat=None, frame_off=None, keys=None, kstat=None, ref_istat=None):
        s, D = w.s, w.D
        self.out = s.out if out is None else out
        self.istat = istat                      # index_status of the frame table
        self.ref_istat = istat if ref_istat is None else ref_istat   # of the reference (a key kill among them)
        self.frame_off = s.frame_off if frame_off is None else frame_off
        self.keys = s.keys if keys is None else keys
        self.table = w.table if out is None else D.stream_table(self.out, s.off, s.olen, s.hashes, s.pads, s.cls)
        self.frames = D.frame_table(s.fmt, s.cls, s.pads, self.frame_off, s.idx_off, s.nframes, SIZES,
                                    index_status=istat)
        self.ktab = D.key_table(self.keys, s.ivs, kstat) if s.fmt == 15 else None
        w.torch.cuda.synchronize()


class World:
    """The resident streams of test_gpu_fread at one format, their tables, and the damaged and killed variants."""

    def __init__(self, fmt):
        import torch
        from carbonado_amd import device as D
        self.torch, self.D, self.fmt = torch, D, fmt
        self.s = s = F.streams(fmt)
        self.table = D.stream_table(s.out, s.off, s.olen, s.hashes, s.pads, s.cls)
        self.host = s.out.cpu().numpy().copy()
        self._variants = {}

    def variant(self, name) -> Variant:
        if name not in self._variants:
            self._variants[name] = self._make(name)
        return self._variants[name]

    def _make(self, name) -> Variant:
        s = self.s
        if name == "intact":
            return Variant(self)
        C = s.cls[BIG]
        x = s.shift + s.index[BIG][2] + 2000      # inside frame 2's raw bytes
        if name == "flipped":                     # the primary copy damaged inside a frame
            return Variant(self, out=s.damaged(BIG, [x]))
        if name == "five":                        # the same chunk damaged in its primary and the four parity shards
            return Variant(self, out=s.damaged(BIG, [i * C + x % C for i in (x // C, 4, 5, 6, 7)]))
        if name == "two":                         # two shards damaged in the same chunks: still rebuilt
            return Variant(self, out=s.damaged(BIG, [i * C + x % C for i in (x // C, 5)]))
        if name == "parent":                      # the CV of a chunk of frame 2 flipped in its parent: the chunk is
            c = (x // 1024) & ~1                  # rebuilt under a path that does not hold (unvouched; 7 under STRICT)
            return Variant(self, out=s.flipped([s.chunk_pos(BIG, c, 0) - 64 + 5]))
        if name == "killed":                     # index_status words; the killed streams' indexes are not looked at
            istat = [0] * s.count
            istat[KILLED_11], istat[KILLED_5] = UNSUPPORTED, HASH
            fo = s.frame_off.copy()
            for k in (KILLED_11, KILLED_5):
                fo[s.idx_off[k]:s.idx_off[k] + s.nframes[k] + 1] = 0
            return Variant(self, istat=istat, frame_off=fo)
        if name == "keykilled":                   # 15: a key_status word, and an index_status word beside it
            kstat, istat = [0] * s.count, [0] * s.count
            kstat[KEY_KILLED], istat[KILLED_5] = KEY_KILL, HASH
            ref = list(istat)
            ref[KEY_KILLED] = KEY_KILL
            return Variant(self, istat=istat, kstat=kstat, ref_istat=ref)
        if name == "wrongkey":
            keys, _, kstat = self.D.stream_keys(bytes(range(3, 35)), s.out, s.off, s.olen, s.hashes, s.pads, s.cls,
                                                self.D.stream_keys_scratch(s.count))
            assert not kstat.any() and not np.array_equal(keys, s.keys)
            return Variant(self, keys=keys)
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def world(fmt) -> World:
    return World(fmt)


def base_requests(m):
    """[(stream, start, len, refused)] in plaintext bytes for a capacity of m bytes per request."""
    P = SIZES[BIG]
    c = lambda n: min(n, m)
    out = [(BIG, 2 * FRAME - c(2 * FRAME), c(2 * FRAME), 0),           # ends on a frame boundary
           (BIG, FRAME, m, 0),                                         # starts on one
           (BIG, FRAME - min((m + 1) // 2, FRAME), m, 0),              # straddles one (m = 1: starts on it)
           (BIG, FRAME - 1, m, 0),                                     # one byte of frame 0; 3 frames from 65538 on
           (BIG, 2 * FRAME - 1, c(2), 0), (BIG, 3 * FRAME - c(100), c(5000), 0),   # raw frames into the short last one
           (BIG, 2 * FRAME + 17, c(300), 0), (6, FRAME - 1, c(6), 0), (6, 2 * FRAME, c(5), 0),
           (TWO_RAW, 12345, m, 0), (3, 4096, c(4096), 0), (4, FRAME, 1, 0)]
    for s, Ps in enumerate(SIZES):
        out += [(s, 0, m, 0), (s, 0, 1, 0),                            # from the start; clipped at plain_len where short
                (s, max(Ps - 1, 0), 1, 0), (s, Ps, 10, 0), (s, Ps + 5, m, 0),    # at plain_len - 1, at it, beyond it
                (s, min(3, Ps), 0, 0),                                 # len 0
                (s, max(Ps - 1, 0), m + 5, 0)]                         # clipped at the end
    out += [(BIG, P - m, m + 7, 0),                                    # a clipped length of max_len
            (BIG, P - m - 1, m + 7, REFUSED), (BIG, 0, m + 1, REFUSED),  # and of max_len + 1
            (len(SIZES), 0, 1, REFUSED), (BIG, (1 << 53) + 1, 1, REFUSED), (BIG, 0, (1 << 53) + 1, REFUSED),
            (BIG, 1 << 53, 1 << 53, 0)]                                # the largest start and len: beyond, empty
    out += [(BIG, 70000 + 17 * k, c(33 + k), 0) for k in range(16)]    # start residues
    return out


def _requests(nreq, m):
    base = base_requests(m)
    return [base[(r + 9) % len(base)] for r in range(nreq)]


class Planned(RW.Planned):
    def __init__(self, w, nreq, max_len, variant="intact", table=None, frames=None):
        self.v = w.variant(variant)
        self.frames = frames or self.v.frames
        super().__init__(w, nreq, max_len, table=table or self.v.table)

    def scratch_len(self):
        return self.w.D.planned_frame_read_scratch(self.table, self.frames, self.nreq, self.max_len).numel()

    def enqueue(self, flags=0):
        self.w.D.read_frame_ranges_planned(self.table, self.frames, self.v.ktab, self.rs, self.start, self.length,
                                           self.max_len, self.content, self.stride, self.clen, self.status, self.used,
                                           self.vouch, self.scratch, flags)


@functools.lru_cache(maxsize=None)
def _reference(fmt, variant, reqs, stride, flags) -> Got:
    w = world(fmt)
    torch, D, s, v = w.torch, w.D, w.s, w.variant(variant)
    n = len(reqs)
    rs, start, length, coff = RW.host_requests(reqs, stride)
    _, _, _, nseg, stage, vseg = D.frame_read_layout(fmt, s.cls, s.pads, v.frame_off, s.idx_off, s.nframes, SIZES, rs,
                                                     start, length, index_status=v.ref_istat)
    content = torch.full((n * stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
    status, used, vouch = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    clen = D.read_frame_ranges(fmt, v.out, s.off, s.olen, s.hashes, s.pads, s.cls, v.frame_off, s.idx_off, s.nframes,
                               SIZES, rs, start, length, content, coff, status, used, vouch,
                               D.frame_read_scratch(n, nseg, stage, vseg, s.count), flags=flags, keys=v.keys, ivs=s.ivs,
                               index_status=v.ref_istat)
    return RW.host_result(reqs, clen, content, status, used, vouch)


def reference(w: World, reqs, stride, flags=0, variant="intact") -> Got:
    """The host-planned call over the same requests at r * stride (computed once
    per request set); a refused request reads an empty range there and has
    status 1, used 0, vouch 0 here."""
    return _reference(w.fmt, variant, tuple(reqs), stride, flags)


def _plain(w, r, rq, got, stride):
    s, start, ln, _ = rq
    want = np.frombuffer(w.s.pt[s][start:start + ln], dtype=np.uint8)
    assert got.status[r] == 0 and got.clen[r] == want.size, rq
    assert np.array_equal(got.content[r * stride:r * stride + want.size], want), rq


@pytest.mark.parametrize("fmt", FORMATS)
def test_base_set_is_what_it_says(gpu, fmt):
    """The reference itself, against the test's own plaintexts, and the shapes the set claims."""
    w = world(fmt)
    for m in (1, 4096, 65537, 70000):
        reqs = base_requests(m)
        stride = RW.up16(m) + 16
        ref = reference(w, reqs, stride)
        for r, rq in enumerate(reqs):
            if not rq[3]:
                _plain(w, r, rq, ref, stride)
        frames = [(a // FRAME, (min(a + n, SIZES[s]) - 1) // FRAME) for s, a, n, f in reqs
                  if not f and n and a < SIZES[s]]
        assert max(f1 - f0 for f0, f1 in frames) + 1 == (m + 65534) // 65536 + 1 == {1: 1, 4096: 2, 65537: 2, 70000: 3}[m]
        assert m in ref.clen and sum(rq[3] for rq in reqs) == 5


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("max_len", [1, 4096, 65537, 70000])
@pytest.mark.parametrize("nreq", [1, 63, 64, 65, 257])
def test_planned_equals_host_planned(gpu, fmt, nreq, max_len):
    w = world(fmt)
    reqs = _requests(nreq, max_len)
    assert nreq < 63 or sum(r[3] for r in reqs) >= 2
    p = Planned(w, nreq, max_len)
    for flags in (0, STRICT):
        got = p.run(reqs, flags)
        assert_equal(got, reference(w, reqs, p.stride, flags), reqs)
        for r, rq in enumerate(reqs):                                  # and the test's own plaintexts
            if not rq[3]:
                _plain(w, r, rq, got, p.stride)
    assert np.array_equal(w.s.out.cpu().numpy(), w.host), "a read changed the streams"


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_request_alone(gpu, fmt):
    """Capacity 1, each request of the base set in turn: the result it has inside the batch."""
    w = world(fmt)
    base = base_requests(4096)
    p = Planned(w, 1, 4096)
    batch = reference(w, base, p.stride)
    for r, rq in enumerate(base):
        got = p.run([rq])
        assert_equal(got, reference(w, [rq], p.stride), [rq])
        assert (got.status[0], got.used[0], got.vouch[0], got.clen[0]) == (batch.status[r], batch.used[r],
                                                                          batch.vouch[r], batch.clen[r]), rq
        assert np.array_equal(got.content[:p.stride], batch.content[r * p.stride:(r + 1) * p.stride]), rq


def _big_requests():
    return [(BIG, 2 * FRAME + 1000, 300, 0), (BIG, 10, 100, 0), (BIG, 3 * FRAME + 5, 50, 0), (3, 100, 4000, 0),
            (BIG, SIZES[BIG] - 1, 1, 0), (BIG, 2 * FRAME - 10, 4096, 0), (BIG, 0, 4097, REFUSED)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_damage_is_rebuilt_and_vouched_for_or_fails_alone(gpu, fmt):
    w = world(fmt)
    reqs = _big_requests()
    for variant in ("flipped", "two", "five", "parent"):
        p = Planned(w, len(reqs), 4096, variant=variant)
        for flags in (0, STRICT):
            got = p.run(reqs, flags)
            assert_equal(got, reference(w, reqs, p.stride, flags, variant), reqs)
            if variant == "five":      # 7 and zeros for the requests over the chunk, the stream's others served
                assert got.status.tolist() == [ZFEC, 0, 0, 0, 0, ZFEC, 1]
                assert got.used[0] == 0 and got.vouch[0] == 0 and not got.content[:300].any()
            elif variant == "parent":  # handed out unvouched; refused under CHIPV_STRICT
                want = ZFEC if flags else 0
                assert got.status.tolist() == [want, 0, 0, 0, 0, want, 1]
                assert got.vouch[0] & UNVOUCHED and got.vouch[5] & UNVOUCHED and not got.vouch[1:5].any()
            else:                      # rebuilt from four other shards and vouched for
                assert got.status.tolist() == [0] * 6 + [1] and got.vouch.tolist() == [VOUCHED, 0, 0, 0, 0, VOUCHED, 0]
                assert variant == "two" or bin(got.used[0]).count("1") == 4
                for r, rq in enumerate(reqs[:6]):
                    _plain(w, r, rq, got, p.stride)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_stream_killed_by_its_index(gpu, fmt):
    w = world(fmt)
    reqs = _requests(129, 4096) + [(KILLED_5, 5, 10, 0), (KILLED_5, 0, 0, 0), (KILLED_11, 0, 4097, REFUSED)]
    p = Planned(w, len(reqs), 4096, variant="killed")
    got = p.run(reqs)
    assert_equal(got, reference(w, reqs, p.stride, 0, "killed"), reqs)
    kill = {KILLED_11: UNSUPPORTED, KILLED_5: HASH}
    seen = set()
    for r, (s, a, n, refused) in enumerate(reqs):
        if s in kill and not refused:   # the word, zeros over the clipped length, even for an empty request
            want = len(w.s.pt[s][a:a + n])
            assert (got.status[r], got.used[r], got.vouch[r], got.clen[r]) == (kill[s], 0, 0, want)
            assert not got.content[r * p.stride:r * p.stride + want].any()
            seen.add((s, want > 0))
        elif not refused:
            _plain(w, r, reqs[r], got, p.stride)
    assert seen == {(KILLED_11, True), (KILLED_11, False), (KILLED_5, True), (KILLED_5, False)}


def test_a_stream_killed_by_its_key_and_a_wrong_key(gpu):
    w = world(15)
    reqs = _requests(129, 4096)
    p = Planned(w, len(reqs), 4096, variant="keykilled")
    got = p.run(reqs)
    assert_equal(got, reference(w, reqs, p.stride, 0, "keykilled"), reqs)
    mine = [r for r, rq in enumerate(reqs) if rq[0] == KEY_KILLED and not rq[3]]
    assert mine and all(got.status[r] == KEY_KILL and got.used[r] == 0 and got.vouch[r] == 0 for r in mine)
    assert any(got.clen[r] for r in mine) and any(got.status[r] == HASH for r in range(len(reqs)))
    # a wrong key: the frames do not agree with the index, 16 and zeros; empty requests are served
    p = Planned(w, len(reqs), 4096, variant="wrongkey")
    got = p.run(reqs)
    assert_equal(got, reference(w, reqs, p.stride, 0, "wrongkey"), reqs)
    for r, rq in enumerate(reqs):
        if not rq[3]:
            assert got.status[r] == (SNAP if got.clen[r] else 0), rq
            assert not got.content[r * p.stride:r * p.stride + got.clen[r]].any(), rq


def _touched(s, rq):
    st, a, n, refused = rq
    if refused or not n or a >= SIZES[st]:
        return []
    e = min(a + n, SIZES[st])
    return [s.index[st][f + 1] - s.index[st][f] for f in range(a // FRAME, (e - 1) // FRAME + 1)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_lying_tables_refuse_exactly_their_requests(gpu, fmt):
    from carbonado_amd import _lib
    w = world(fmt)
    s, D, v = w.s, w.D, w.variant("intact")
    reqs = _requests(129, 4096)
    fi, ti = v.frames.info, v.table.info
    assert fi.max_frame == FRAME + 8 and fi.nentries == sum(n + 1 for n in s.nframes) and fi.format == fmt

    def check(marked, **kw):
        assert 0 < sum(m[3] and not r[3] for m, r in zip(marked, reqs)) < sum(not r[3] for r in reqs)
        got = Planned(w, len(reqs), 4096, **kw).run(reqs)
        assert_equal(got, reference(w, marked, RW.up16(4096) + 16), marked)

    # a max_frame below a touched frame: the requests over a full raw frame
    lying = D.FrameTable(v.frames.table, _lib.FrameInfo(fi.nstreams, fi.nentries, fi.max_frame - 1, fmt))
    check([(a, b, c, REFUSED if f or max(_touched(s, (a, b, c, f)), default=0) > fi.max_frame - 1 else 0)
           for a, b, c, f in reqs], frames=lying)
    # an nentries below the last stream's entries: that stream's requests
    lying = D.FrameTable(v.frames.table, _lib.FrameInfo(fi.nstreams, fi.nentries - 1, fi.max_frame, fmt))
    check([(a, b, c, REFUSED if a == BIG else f) for a, b, c, f in reqs], frames=lying)
    # an info that contradicts a stream record: the streams of the most chunks
    lying = D.StreamTable(v.table.table, _lib.TableInfo(ti.nstreams, ti.max_chunks - 1, ti.min_shard, 0))
    most = {o for o, c in enumerate(s.cls) if 8 * c // 1024 == ti.max_chunks}
    assert most and len(most) < s.count
    check([(a, b, c, REFUSED if a in most else f) for a, b, c, f in reqs], table=lying)


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay_with_requests_rewritten_in_place(gpu, fmt):
    w = world(fmt)
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
    first = [(BIG, 1000, 4096, 0), (BIG, 1000, 0, 0), (BIG, 1000, 4097, REFUSED)]   # slot 0: read, empty, refused
    for k in range(3):
        reqs = [first[k]] + [base[(7 * k + 3 * r + 1) % len(base)] for r in range(1, nreq)]
        assert any(r[3] for r in reqs[1:]) and any(len(_touched(w.s, r)) == 2 for r in reqs)
        p.set(reqs)
        p.clen.fill_(-1); p.status[:nreq].fill_(-1); p.used[:nreq].fill_(-1); p.vouch[:nreq].fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        got = p.result()
        assert_equal(got, reference(w, reqs, p.stride), reqs)
        assert (got.status[0], got.clen[0]) == ((0, 4096), (0, 0), (1, 0))[k]


@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_table_holds_what_the_layout_says(gpu, fmt):
    from carbonado_amd import _lib
    w = world(fmt)
    s = w.s
    for variant, killed in (("intact", ()), ("killed", (KILLED_11, KILLED_5))):
        v = w.variant(variant)
        img = v.frames.table.cpu().numpy()
        live = [o for o in range(s.count) if o not in killed]
        ne = sum(s.nframes[o] + 1 for o in live)
        assert (v.frames.nstreams, v.frames.nentries, v.frames.max_frame, v.frames.format) == (s.count, ne, FRAME + 8, fmt)
        assert img.size >= 32 * s.count + RW.up16(8 * ne) == _lib.lib().chipg_frame_table_len(s.count, ne)
        recs = img[:32 * s.count].view(np.uint64).reshape(s.count, 4)
        entries = img[32 * s.count:32 * s.count + 8 * ne].view(np.uint64)
        e = 0
        for o in range(s.count):
            if o in killed:
                assert recs[o].tolist() == [0, 0, SIZES[o], v.istat[o]]
                continue
            assert recs[o].tolist() == [e, s.nframes[o], SIZES[o], 0]
            assert entries[e:e + s.nframes[o] + 1].tolist() == s.index[o]
            e += s.nframes[o] + 1
        assert e == ne
