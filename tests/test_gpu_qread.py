"""The device-planned ranged reads (include/carbonado_hip_qread.h) against the
host-planned ones: for every request set, content, content length, status,
used and vouch of read_ranges_planned / read_ranges_vouched_planned equal
read_ranges / read_ranges_vouched of the same requests placed at r * stride.
What the host-planned calls refuse for a whole call (a stream index past the
table, a range above 2^53) and what they have no word for (content longer than
the capacity) is status 1 per request here; the reference reads an empty range
in that request's place.

Streams are level-12 encodings made on the device (encode_ragged) with shard
lengths 1024 (objects of 1, 1000, 4000 and 4096 bytes), 2048, 4096 and 65536,
with and without padding, one described with a chunk_len that does not fit, and
damaged ones: a flipped bit in a primary chunk (rebuilt), five shards damaged
(7), a damaged parent above a rebuilt chunk (unvouched), and a stream over
shards that are no valid zfec encoding (5).  The content buffer is filled with
a canary and only [0, content_len[r]) of a slot may change; the scratch carries
guard bytes behind the length the call is told."""
import functools

import numpy as np
import pytest

import read_world as RW  # tests/read_world.py (tests/ is on sys.path under pytest)
from bao_damage import chunk_off
from read_world import CANARY, Got, assert_equal

pytestmark = pytest.mark.gpu

SO = 56
# objects 0..5 intact; 6 described with a chunk_len that does not fit; 7..10 damaged
SIZES = [1, 1000, 4096, 8000, 16384, 262044, 4096, 4000, 4000, 4096, 4096]
MISFIT, FLIPPED, FIVE, PARENT, CONTRA = 6, 7, 8, 9, 10
SHARD = [1024, 1024, 1024, 2048, 4096, 65536, 1024, 1024, 1024, 1024, 1024]
REFUSED = 1


class World:
    """The resident streams, made once."""

    def __init__(self):
        import torch
        from carbonado_amd import device as D
        self.torch, self.D = torch, D
        count = len(SIZES)
        torch.manual_seed(11)
        pitch = 1 << 18
        self.inp = torch.randint(0, 256, (count * pitch,), dtype=torch.uint8, device="cuda")
        in_off = [o * pitch for o in range(count)]
        self.off, self.len, total = D.ragged_layout(12, SIZES, 256, SO)
        self.buf = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        _, infos = D.encode_ragged(12, self.inp, in_off, SIZES, self.buf, self.off, self.hashes,
                                   D.ragged_scratch(12, SIZES))
        self.pads = [i.padding_len for i in infos]
        self.cls = [i.chunk_len for i in infos]
        assert self.cls == SHARD and self.pads[2] == 0 and self.pads[0] == 4095 and self.pads[5] == 100
        # the contradiction: zfec, one byte of parity shard 4 altered, then bao over the eight shards as they are
        zoff, zlen, ztotal = D.ragged_layout(8, [SIZES[CONTRA]], 256, 0)
        z = torch.zeros(ztotal, dtype=torch.uint8, device="cuda")
        zh = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
        zl, _ = D.encode_ragged(8, self.inp, [in_off[CONTRA]], [SIZES[CONTRA]], z, zoff, zh, D.ragged_scratch(8, [4096]))
        assert zl == [8192]
        z[zoff[0] + 4 * 1024 + 10] ^= 0x01
        boff, blen, btotal = D.ragged_layout(4, [8192], 256, SO)
        b = torch.zeros(btotal, dtype=torch.uint8, device="cuda")
        bl, _ = D.encode_ragged(4, z, [zoff[0]], [8192], b, boff, self.hashes[CONTRA:CONTRA + 1],
                                D.ragged_scratch(4, [8192]))
        assert bl == [self.len[CONTRA]]
        self.buf[self.off[CONTRA]:self.off[CONTRA] + bl[0]] = b[boff[0]:boff[0] + bl[0]]
        torch.cuda.synchronize()
        self.objects = [self.inp[o:o + n].cpu().numpy() for o, n in zip(in_off, SIZES)]
        self.cls[MISFIT] = 2048
        # damage (streams of 8 chunks: chunk i = shard i)
        flips = [(FLIPPED, chunk_off(1, 8) + 300), (CONTRA, chunk_off(0, 8) + 700),
                 (PARENT, chunk_off(2, 8) - 64 + 5)]  # the CV of chunk 2 in the parent over chunks 2 and 3
        flips += [(FIVE, chunk_off(i, 8) + 40 + i) for i in (1, 0, 4, 6, 2)]
        at = torch.tensor([self.off[s] + o for s, o in flips], dtype=torch.int64, device="cuda")
        self.buf[at] ^= 0x10
        torch.cuda.synchronize()
        self.host = self.buf.cpu().numpy().copy()
        self.table = D.stream_table(self.buf, self.off, self.len, self.hashes, self.pads, self.cls)
        torch.cuda.synchronize()
        assert (self.table.nstreams, self.table.max_chunks, self.table.min_shard) == (count, 512, 1024)


@functools.lru_cache(maxsize=None)
def world() -> World:
    return World()


def base_requests(max_len):
    """[(stream, start, len, refused)]"""
    n5 = SIZES[5]
    out = [(2, 100, 200, 0)]                                             # inside one chunk
    out += [(3, 1024 + k, 300 + k, 0) for k in range(16)]                # every start residue mod 16
    out += [(3, 1000, 100, 0), (5, 2 * 65536 + 1020, 10, 0), (4, 4090, 12, 0)]  # across a chunk / a shard boundary
    out += [(2, 1000, 100, 0), (2, 1000, 1100, 0), (2, 1000, 2100, 0), (2, 0, 4096, 0), (2, 1023, 3073, 0)]  # 1, 2, 3 shard boundaries
    out += [(2, 5, 0, 0), (1, 1000, 10, 0), (1, 5000, 1, 0), (0, 1, 1, 0)]  # len 0, start >= n_obj
    out += [(1, 990, 100, 0), (0, 0, 50, 0), (5, n5 - 50, 4096, 0), (3, 7990, max_len, 0)]  # clipped at n_obj
    out += [(5, 65536 - 2000, max_len, 0), (4, 4096 * 2 - 7, max_len, 0), (3, 3, max_len, 0)]  # the whole capacity
    out += [(4, 0, max_len + 1, REFUSED), (5, 17, 1 << 40, REFUSED)]     # content longer than max_len
    out += [(len(SIZES), 0, 10, REFUSED), (2, (1 << 53) + 1, 10, REFUSED), (2, 0, (1 << 53) + 1, REFUSED)]
    out += [(MISFIT, 0, 100, 0)]                                         # chunk_len does not fit: 7
    out += [(FLIPPED, 1024 + 100, 200, 0), (FLIPPED, 1000, 1500, 0), (FLIPPED, 2048, 100, 0)]
    out += [(FIVE, 1024 + 10, 50, 0), (FIVE, 3072, 20, 0)]
    out += [(PARENT, 2048 + 10, 100, 0), (PARENT, 0, 4096, 0)]
    out += [(CONTRA, 5, 100, 0), (CONTRA, 1024, 100, 0)]
    return out


class Planned(RW.Planned):
    def __init__(self, w: World, nreq, max_len, vouched, table=None):
        self.vouched = vouched
        super().__init__(w, nreq, max_len, table)

    def scratch_len(self):
        return self.w.D.planned_read_scratch(self.table, self.nreq, self.max_len, self.vouched).numel()

    def enqueue(self, flags=0):
        D = self.w.D
        if self.vouched:
            D.read_ranges_vouched_planned(self.table, self.rs, self.start, self.length, self.max_len, self.content,
                                          self.stride, self.clen, self.status, self.used, self.vouch, self.scratch, flags)
        else:
            D.read_ranges_planned(self.table, self.rs, self.start, self.length, self.max_len, self.content, self.stride,
                                  self.clen, self.status, self.used, self.scratch)


def reference(w: World, reqs, max_len, stride, vouched, flags=0, content=None, content_base=0) -> Got:
    """The host-planned call over the same requests at r * stride; a refused
    request reads an empty range there and has status 1, used 0, vouch 0 here.
    `content`: a canary-filled buffer of the caller's, request r at
    content_base + r * stride of it (w is then any object with World's fields)."""
    torch, D = w.torch, w.D
    n = len(reqs)
    rs, start, length, coff = RW.host_requests(reqs, stride)
    _, _, _, nseg = D.read_layout(w.cls, w.pads, rs, start, length, 16)
    if content is None:
        content = torch.full((n * stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
    coff = [content_base + c for c in coff]
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    used = torch.zeros(n, dtype=torch.int32, device="cuda")
    vouch = torch.zeros(n, dtype=torch.int32, device="cuda")
    if vouched:
        clen = D.read_ranges_vouched(w.buf, w.off, w.len, w.hashes, w.pads, w.cls, rs, start, length, content, coff,
                                     status, used, vouch, D.vread_scratch(n, nseg), flags)
    else:
        clen = D.read_ranges(w.buf, w.off, w.len, w.hashes, w.pads, w.cls, rs, start, length, content, coff, status, used,
                             D.read_scratch(n, nseg))
    return RW.host_result(reqs, clen, content[content_base:content_base + n * stride + 64], status, used,
                          vouch if vouched else None)


def _requests(nreq, max_len):
    base = base_requests(max_len)
    return [base[(r + nreq) % len(base)] for r in range(nreq)]


def check_base_set(w, reference, max_lens=(4096, 5000)):
    """The host-planned calls over the base set: the clean objects' bytes, and
    every damage class is there.  reference(w, reqs, max_len, stride, vouched
    [, flags]) is the function above, or it with a content buffer of the caller's."""
    for max_len in max_lens:
        reqs = base_requests(max_len)
        stride = (max_len + 15) // 16 * 16 + 16
        ref = reference(w, reqs, max_len, stride, True)
        by = {rq[:3]: r for r, rq in enumerate(reqs)}
        for r, (s, start, ln, refused) in enumerate(reqs):
            if refused or s in (MISFIT, FIVE, CONTRA):
                continue
            want = w.objects[s][start:start + ln]
            assert ref.clen[r] == len(want) and ref.status[r] == 0
            assert np.array_equal(ref.content[r * stride:r * stride + len(want)], want), reqs[r]
        assert ref.clen[by[2, 0, 4096]] == 4096 and ref.used[by[2, 0, 4096]] == 0b1111
        assert ref.status[by[MISFIT, 0, 100]] == 7
        r = by[FLIPPED, 1124, 200]
        assert (ref.status[r], ref.used[r], ref.vouch[r]) == (0, 0b11101, 1)            # rebuilt and vouched
        assert ref.used[by[FLIPPED, 2048, 100]] == 0b100                                # not the damaged primary
        assert ref.status[by[FIVE, 1034, 50]] == 7 and ref.status[by[FIVE, 3072, 20]] == 0
        r = by[PARENT, 2058, 100]
        assert (ref.status[r], ref.vouch[r]) == (0, 2) and ref.used[r] == 0b110011      # unvouched; shard 3 shares the parent
        assert reference(w, reqs, max_len, stride, True, 1).status[r] == 7              # strict
        r = by[CONTRA, 5, 100]
        assert (ref.status[r], ref.vouch[r], ref.used[r]) == (5, 4, 0)
        assert not ref.content[r * stride:r * stride + 100].any()
        assert ref.status[by[CONTRA, 1024, 100]] == 0
        plain = reference(w, reqs, max_len, stride, False)
        assert plain.status[by[CONTRA, 5, 100]] == 0 and plain.status[by[PARENT, 2058, 100]] == 0


def test_base_set_is_what_it_says(gpu):
    """The reference itself: the clean objects' bytes, and every damage class is there."""
    check_base_set(world(), reference)


# 512: S = 4 slots per request, so 2049 entries per prefix array: three scan workgroups of 1024 entries, and one
# entry more than a whole number of them; 257: two workgroups
@pytest.mark.parametrize("max_len", [4096, 5000])
@pytest.mark.parametrize("nreq", [1, 63, 64, 65, 257, 512])
def test_planned_equals_host_planned(gpu, nreq, max_len):
    w = world()
    reqs = _requests(nreq, max_len)
    assert nreq < 63 or sum(r[3] for r in reqs) >= 5
    p = Planned(w, nreq, max_len, False)
    assert_equal(p.run(reqs), reference(w, reqs, max_len, p.stride, False), reqs)
    v = Planned(w, nreq, max_len, True)
    for flags in (0, w.D.VREAD_STRICT):
        assert_equal(v.run(reqs, flags), reference(w, reqs, max_len, v.stride, True, flags), reqs)
    assert np.array_equal(w.buf.cpu().numpy(), w.host), "a read changed the streams"


def test_every_request_alone(gpu):
    """Capacity 1, each request of the base set in turn: the last slot is the first."""
    w = world()
    p, v = Planned(w, 1, 4096, False), Planned(w, 1, 4096, True)
    for rq in base_requests(4096):
        assert_equal(p.run([rq]), reference(w, [rq], 4096, p.stride, False), [rq])
        assert_equal(v.run([rq]), reference(w, [rq], 4096, v.stride, True), [rq])


def test_lying_info_refuses_that_streams_requests(gpu):
    w = world()
    from carbonado_amd import _lib
    info = _lib.TableInfo(w.table.info.nstreams, w.table.info.max_chunks - 1, w.table.info.min_shard, 0)
    lying = w.D.StreamTable(w.table.table, info)
    reqs = _requests(64, 4096)
    assert any(r[0] == 5 and not r[3] for r in reqs)
    got = Planned(w, 64, 4096, True, table=lying).run(reqs)
    # stream 5 alone has 512 chunks: its requests are refused, every other request is as before
    marked = [(s, a, b, REFUSED if s == 5 else f) for s, a, b, f in reqs]
    assert_equal(got, reference(w, marked, 4096, (4096 + 15) // 16 * 16 + 16, True), marked)


def test_graph_replay_with_requests_rewritten_in_place(gpu):
    w = world()
    torch = w.torch
    nreq, max_len = 65, 4096
    p = Planned(w, nreq, max_len, False)
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
        reqs = [base[(5 * k + 3 * r + 1) % len(base)] for r in range(nreq)]
        p.set(reqs)
        p.clen.fill_(-1); p.status[:nreq].fill_(-1); p.used[:nreq].fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        assert_equal(p.result(), reference(w, reqs, max_len, p.stride, False), reqs)
