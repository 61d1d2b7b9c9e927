"""The device-planned slice audits (include/carbonado_hip_paudit.h,
carbonado_amd.device verify_slices_planned / extract_slices_planned /
verify_slice_proofs_planned) against the host-planned ones: for every request
set, the proof bytes, proof length, status, content and content length equal
what extract_slices / verify_slices / verify_slice_proofs give the same
requests placed at r * stride.  What the host-planned calls refuse for a whole
call or have no word for (a stream index past the table, more chunks than the
capacity) is status 1 per request here and left out of the reference's set; a
proof of the wrong length is status 6.  The clean results are also the Python
oracle's (oracle/pyoracle.py: bao_slice, bao_decode_slice).

Streams are built and packed as in tests/test_gpu_audit.py (one buffer, at 56
and 8 mod 256).  Every output buffer is filled with a canary and compared
WHOLE with the reference's, on the device: only bytes [0, len) of a served slot
may change, nothing between slots, past nreq or past scratch_len."""
import functools
import random

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from test_gpu_audit import DAMAGE_SIZES, _pack_streams, _stream
from test_slice_verify import _grid
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 1023, 1024, 1025, 3072, 5121, 8192, 8193, 13317, 24576, 66561]
COUNTS = [1, 2, 3, 8, 70]
CANARY = 0xA5
GUARD = 4096
BIG = 1 << 53
SPARE = 0xFFFFFFFF
REFUSED, MISMATCH, TRUNCATED = 1, 5, 6


def chunks(n: int) -> int:
    return max(1, -(-n // 1024))


def selected(n: int, index: int, count: int) -> int:
    N = chunks(n)
    first = min(index, N - 1)
    return max(min(index + count, N), first + 1) - first


class World:
    """Resident streams, their stream table (the holder's) and root table (the auditor's)."""

    def __init__(self, blobs, ns, hashes):
        import torch
        from carbonado_amd import device as D
        self.torch, self.D = torch, D
        self.blobs, self.ns, self.hash_list = blobs, list(ns), hashes
        host, self.in_off = _pack_streams(blobs)
        self.in_len = [len(b) for b in blobs]
        self.streams = torch.from_numpy(host).cuda()
        self.hashes = torch.from_numpy(np.frombuffer(b"".join(hashes), dtype=np.uint8).copy()).cuda()
        k = len(blobs)
        self.table = D.stream_table(self.streams, self.in_off, self.in_len, self.hashes, [0] * k, [1024] * k)
        self.roots = D.root_table(self.ns, self.hashes)
        torch.cuda.synchronize()
        self.max_chunks = max(chunks(n) for n in ns)
        assert (self.table.nstreams, self.table.max_chunks) == (k, self.max_chunks)
        assert (self.roots.nroots, self.roots.max_chunks) == (k, self.max_chunks)

    def strides(self, max_count):
        """(content stride, proof stride): the least the call takes and one unit more, so slots have gaps"""
        bound = self.D.proof_bound(self.max_chunks, max_count)
        return 1024 * max_count + 16, -(-bound // 16) * 16 + 16

    def refused(self, rq, max_count) -> bool:
        s, i, c = rq
        return s != SPARE and (s >= len(self.ns) or i > BIG or c > BIG or selected(self.ns[s], i, c) > max_count)


@functools.lru_cache(maxsize=None)
def world() -> World:
    streams = [_stream(n) for n in SIZES]
    return World([e for _, e, _ in streams], SIZES, [h for _, _, h in streams])


def all_requests():
    """Every (stream, index, count) of _grid, an index past the end, count 0 and count 2^53."""
    reqs = []
    for s, n in enumerate(SIZES):
        N = chunks(n)
        reqs += [(s, i, c) for i, c in _grid(n)]
        reqs += [(s, N + 5, 1), (s, N + 5, 0), (s, 0, 0), (s, N - 1, BIG), (s, 0, BIG), (s, BIG, BIG)]
    return reqs


class Result:
    """status and lengths (numpy, nreq entries) and the output buffer (device, whole)."""

    def __init__(self, status, length, buf):
        self.status, self.length, self.buf = status, length, buf


class Planned:
    """The buffers of planned calls of capacity (nreq, max_count) over a world."""

    def __init__(self, w: World, nreq, max_count, table=None, roots=None):
        t = self.torch = w.torch
        self.w, self.nreq, self.max_count = w, nreq, max_count
        self.table, self.roots = table or w.table, roots or w.roots
        self.cs, self.ps = w.strides(max_count)
        self.rs = t.zeros(nreq, dtype=t.int32, device="cuda")
        self.idx = t.zeros(nreq, dtype=t.int64, device="cuda")
        self.cnt = t.zeros(nreq, dtype=t.int64, device="cuda")
        self.need = w.D.planned_audit_scratch(self.table, nreq, max_count).numel()
        self.scratch = t.full((self.need + GUARD,), CANARY, dtype=t.uint8, device="cuda")
        self.content = t.empty(nreq * self.cs + GUARD, dtype=t.uint8, device="cuda")
        self.proofs = t.empty(nreq * self.ps + GUARD, dtype=t.uint8, device="cuda")
        self.status = t.empty(nreq + 8, dtype=t.int32, device="cuda")
        self.clen = t.empty(nreq + 8, dtype=t.int64, device="cuda")
        self.plen = t.empty(nreq + 8, dtype=t.int64, device="cuda")

    def set(self, reqs):
        t = self.torch
        assert len(reqs) == self.nreq
        self.rs.copy_(t.from_numpy(np.array([r[0] for r in reqs], dtype=np.uint32).view(np.int32)))
        self.idx.copy_(t.tensor([r[1] for r in reqs], dtype=t.int64))
        self.cnt.copy_(t.tensor([r[2] for r in reqs], dtype=t.int64))

    def _result(self, length, buf) -> Result:
        self.torch.cuda.synchronize()
        n = self.nreq
        st, ln = self.status.cpu().numpy(), length.cpu().numpy()
        assert (st[n:] == -1).all() and (ln[n:] == -1).all(), "a result array was written past nreq"
        assert bool((self.scratch[self.need:] == CANARY).all()), "scratch written past scratch_len"
        return Result(st[:n].copy(), ln[:n].copy(), buf)

    def enqueue_verify(self):
        self.w.D.verify_slices_planned(self.table, self.rs, self.idx, self.cnt, self.max_count, self.content, self.cs,
                                       self.clen, self.status, self.scratch[:self.need])

    def enqueue_extract(self):
        self.w.D.extract_slices_planned(self.table, self.rs, self.idx, self.cnt, self.max_count, self.proofs, self.ps,
                                        self.plen, self.status, self.scratch[:self.need])

    def enqueue_verify_proofs(self):
        self.w.D.verify_slice_proofs_planned(self.roots, self.rs, self.idx, self.cnt, self.max_count, self.proofs,
                                             self.ps, self.plen, self.content, self.cs, self.clen, self.status,
                                             self.scratch[:self.need])

    def verify(self) -> Result:
        self.content.fill_(CANARY); self.status.fill_(-1); self.clen.fill_(-1)
        self.enqueue_verify()
        return self._result(self.clen, self.content.clone())

    def extract(self) -> Result:
        """The proofs stay in self.proofs and their lengths in self.plen for verify_proofs."""
        self.proofs.fill_(CANARY); self.status.fill_(-1); self.plen.fill_(-1)
        self.enqueue_extract()
        return self._result(self.plen, self.proofs.clone())

    def verify_proofs(self) -> Result:
        self.content.fill_(CANARY); self.status.fill_(-1); self.clen.fill_(-1)
        keep = self.plen.clone()
        self.enqueue_verify_proofs()
        got = self._result(self.clen, self.content.clone())
        assert self.torch.equal(keep, self.plen), "verify_proofs wrote d_proof_len"
        return got


class Reference:
    """The host-planned calls over the served requests of `reqs`, request r at
    r * stride; a refused request has status 1 and a spare one status 0, both
    with lengths 0 and an untouched slot."""

    def __init__(self, w: World, reqs, max_count):
        t, D = w.torch, w.D
        nreq = len(reqs)
        cs, ps = w.strides(max_count)
        keep = [r for r, rq in enumerate(reqs) if rq[0] != SPARE and not w.refused(rq, max_count)]
        rs, idx, cnt = ([reqs[r][k] for r in keep] for k in range(3))
        coff, poff = [r * cs for r in keep], [r * ps for r in keep]
        ns = [w.ns[s] for s in rs]
        _, plen, _, clen, _, _ = D.slice_layout(ns, idx, cnt, 16)
        m = len(keep)
        scratch = D.audit_scratch(max(len(w.blobs), m), m)

        def spread(values, fill):
            out = np.full(nreq, fill, dtype=np.int64)
            out[keep] = values
            return out

        base = np.array([REFUSED if w.refused(rq, max_count) else 0 for rq in reqs], dtype=np.int64)

        def status_of(st):
            out = base.copy()
            out[keep] = st.cpu().numpy()[:m]
            return out

        self.keep = keep
        self.proofs = t.full((nreq * ps + GUARD,), CANARY, dtype=t.uint8, device="cuda")
        D.extract_slices(w.streams, w.in_off, w.in_len, rs, idx, cnt, self.proofs, poff, plen, scratch)
        self.extract = Result(base.copy(), spread(plen, 0), self.proofs)
        results = []
        for from_proofs in (False, True):
            content = t.full((nreq * cs + GUARD,), CANARY, dtype=t.uint8, device="cuda")
            st = t.zeros(max(m, 1), dtype=t.int32, device="cuda")
            if from_proofs:
                per_req = t.from_numpy(np.frombuffer(b"".join(w.hash_list[s] for s in rs) or bytes(32),
                                                     dtype=np.uint8).copy()).cuda()
                got = D.verify_slice_proofs(self.proofs, poff, plen, ns, per_req, idx, cnt, content, coff, st, scratch)
            else:
                got = D.verify_slices(w.streams, w.in_off, w.in_len, w.hashes, rs, idx, cnt, content, coff, st, scratch)
            assert got == clen
            results.append(Result(status_of(st), spread(clen, 0), content))
        self.verify, self.verify_proofs = results
        t.cuda.synchronize()


def assert_same(got: Result, ref: Result, reqs, what):
    for r in np.flatnonzero(got.status != ref.status)[:3]:
        raise AssertionError(f"{what}: status {got.status[r]} != {ref.status[r]} for request {r} {reqs[r]}")
    for r in np.flatnonzero(got.length != ref.length)[:3]:
        raise AssertionError(f"{what}: length {got.length[r]} != {ref.length[r]} for request {r} {reqs[r]}")
    if not bool((got.buf == ref.buf).all()):
        at = int((got.buf != ref.buf).nonzero()[0])
        raise AssertionError(f"{what}: the output buffers differ at byte {at} of {got.buf.numel()}")


def run_all(p: Planned, ref: Reference, reqs):
    p.set(reqs)
    assert_same(p.verify(), ref.verify, reqs, "verify")
    assert_same(p.extract(), ref.extract, reqs, "extract")
    assert_same(p.verify_proofs(), ref.verify_proofs, reqs, "verify_proofs")


@functools.lru_cache(maxsize=None)
def shuffled(seed=3):
    reqs = all_requests()
    random.Random(seed).shuffle(reqs)
    return reqs


@functools.lru_cache(maxsize=None)
def reference_of_all(max_count) -> Reference:
    return Reference(world(), shuffled(), max_count)


@pytest.mark.parametrize("max_count", COUNTS)
def test_planned_equals_host_planned(gpu, max_count):
    w = world()
    reqs = shuffled()
    refused = sum(w.refused(rq, max_count) for rq in reqs)
    assert (refused == 0) == (max_count == 70) and 2 * refused < len(reqs)
    ref = reference_of_all(max_count)
    assert (ref.verify.status[ref.keep] == 0).all() and 0 < ref.verify.length.max() <= 1024 * max_count
    run_all(Planned(w, len(reqs), max_count), ref, reqs)
    assert np.array_equal(w.streams.cpu().numpy(), _pack_streams(w.blobs)[0]), "an audit changed the streams"


def test_clean_results_are_the_oracles(gpu):
    """The reference itself, and so the planned calls: proofs are bao_slice's, content bao_decode_slice's."""
    w = world()
    reqs = shuffled()
    ref = reference_of_all(70)
    cs, ps = w.strides(70)
    proofs, content = ref.extract.buf.cpu().numpy(), ref.verify.buf.cpu().numpy()
    memo = {s: P.bao_prime(w.blobs[s], w.hash_list[s]) for s in range(len(SIZES))}
    assert len(ref.keep) == len(reqs)
    for r, (s, i, c) in enumerate(reqs):
        sl = P.bao_slice(w.blobs[s], i * 1024, c * 1024)
        assert proofs[r * ps:r * ps + ref.extract.length[r]].tobytes() == sl, reqs[r]
        want = P.bao_decode_slice(sl, w.hash_list[s], i * 1024, c * 1024, memo=memo[s])
        assert content[r * cs:r * cs + ref.verify.length[r]].tobytes() == want, reqs[r]
        assert want == _stream(SIZES[s])[0][i * 1024:(i + c) * 1024]


def test_every_request_alone_and_between_spares(gpu):
    """Capacity 1, each request in turn (the last slot is the first), against
    its slot of the batch's reference; then every request with a spare slot on
    either side."""
    w = world()
    t = w.torch
    reqs = shuffled()
    ref = reference_of_all(8)
    cs, ps = w.strides(8)
    one = Planned(w, 1, 8)

    def slot_of(res: Result, r, stride):
        return res.status[r], res.length[r], res.buf[r * stride:(r + 1) * stride]

    for r, rq in enumerate(reqs):
        one.set([rq])
        for got, want, stride in ((one.verify(), ref.verify, cs), (one.extract(), ref.extract, ps),
                                  (one.verify_proofs(), ref.verify_proofs, cs)):
            st, ln, buf = slot_of(want, r, stride)
            assert (got.status[0], got.length[0]) == (st, ln), rq
            assert t.equal(got.buf[:stride], buf) and bool((got.buf[stride:] == CANARY).all()), rq
    spaced = [x for rq in reqs for x in ((SPARE, 5, 5), rq)] + [(SPARE, BIG + 7, BIG + 7)]
    run_all(Planned(w, len(spaced), 8), Reference(w, spaced, 8), spaced)


@pytest.mark.parametrize("n", DAMAGE_SIZES)
def test_every_damaged_node_gives_the_host_planned_verdicts(gpu, n):
    """One stream per damaged node (each parent half, each chunk) and the clean
    stream, the full grid of requests on each, in one call; the proofs of the
    damaged streams are the damaged proofs.  Then proofs of the wrong length."""
    d, enc, h = _stream(n)
    nodes = B.tree_nodes(n)
    rng = random.Random(n)
    blobs = [B.flip(enc, nodes, case, rng) for case in B.every_node_cases(nodes) if nodes[case[0]].size] + [enc]
    w = World(blobs, [n] * len(blobs), [h] * len(blobs))
    t = w.torch
    grid = _grid(n)
    N = chunks(n)
    reqs = [(s, i, c) for s in range(len(blobs)) for i, c in grid]
    ref = Reference(w, reqs, N)
    assert len(ref.keep) == len(reqs)
    failed = int((ref.verify.status == MISMATCH).sum())
    assert 5 * failed >= len(reqs) and 5 * (len(reqs) - failed) >= len(reqs), (failed, len(reqs))
    assert (ref.verify.status[-len(grid):] == 0).all()  # the clean stream, among damaged neighbours
    assert np.array_equal(ref.verify.status, ref.verify_proofs.status)
    p = Planned(w, len(reqs), N)
    run_all(p, ref, reqs)

    # every seventh proof arrives one byte short or long: 6, the content length stated, zeros
    cs, _ = w.strides(N)
    wrong = np.arange(0, len(reqs), 7)
    delta = t.zeros_like(p.plen)
    delta[t.from_numpy(wrong).cuda()] = t.tensor([1 if k % 2 else -1 for k in range(wrong.size)], device="cuda")
    p.plen += delta
    want = Result(ref.verify_proofs.status.copy(), ref.verify_proofs.length, ref.verify_proofs.buf.clone())
    want.status[wrong] = TRUNCATED
    for r in wrong:
        want.buf[r * cs:r * cs + int(want.length[r])] = 0
    assert_same(p.verify_proofs(), want, reqs, "verify_proofs with wrong lengths")


def test_device_refusals_leave_the_neighbours_served(gpu):
    w = world()
    big, mid = SIZES.index(66561), SIZES.index(8192)
    reqs = [(mid, 0, 2), (len(SIZES), 0, 1), (mid, 1, 3), (big, 3, 4), (mid, 2, 1), (0x7FFFFFFF, 0, 1), (big, 60, BIG),
            (mid, BIG + 1, 1), (mid, 0, BIG + 1), (SPARE, 0, 0), (big, 64, 2), (mid, 0, 4), (big, 0, 3)]
    ref = Reference(w, reqs, 3)
    want = [0, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0]
    assert ref.verify.status.tolist() == want and ref.extract.status.tolist() == want
    run_all(Planned(w, len(reqs), 3), ref, reqs)
    # an info that is not the table's: the requests of the stream with the most chunks are refused
    from carbonado_amd import _lib
    ti, ri = w.table.info, w.roots.info
    lying = w.D.StreamTable(w.table.table, _lib.TableInfo(ti.nstreams, ti.max_chunks - 1, ti.min_shard, 0))
    lying_roots = w.D.RootTable(w.roots.table, _lib.RootInfo(ri.nroots, ri.max_chunks - 1))
    marked = [(len(SIZES), i, c) if s == big else (s, i, c) for s, i, c in reqs]  # what the reference leaves out
    assert sum(s == big for s, _, _ in reqs) == 4
    p = Planned(w, len(reqs), 3, table=lying, roots=lying_roots)
    assert (p.cs, p.ps) == w.strides(3)
    run_all_marked = Reference(w, marked, 3)
    p.set(reqs)
    assert_same(p.verify(), run_all_marked.verify, reqs, "verify")
    assert_same(p.extract(), run_all_marked.extract, reqs, "extract")
    assert_same(p.verify_proofs(), run_all_marked.verify_proofs, reqs, "verify_proofs")


def test_graph_replay_with_requests_rewritten_in_place(gpu):
    """verify and extract captured on a side stream after one warm-up (one
    stream: the captured work is one linear chain of six kernels), replayed
    three times with the request arrays rewritten in place; each replay equals
    a fresh host-planned call."""
    w = world()
    torch = w.torch
    nreq, max_count = 65, 8
    base = shuffled()
    v, e = Planned(w, nreq, max_count), Planned(w, nreq, max_count)  # verify's buffers, extract's buffers
    side = torch.cuda.Stream()
    v.set(base[:nreq]); e.set(base[:nreq])
    with torch.cuda.stream(side):
        v.enqueue_verify()  # the warm-up: the thread's context exists from here on
        e.enqueue_extract()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        v.enqueue_verify()
        e.enqueue_extract()
    for k in range(3):
        reqs = [base[(7 * k + 3 * r + 1) % len(base)] for r in range(nreq)]
        reqs[5 + k] = (SPARE, 1, 1)
        for p in (v, e):
            p.set(reqs)
            p.content.fill_(CANARY); p.proofs.fill_(CANARY); p.clen.fill_(-1); p.plen.fill_(-1); p.status.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        ref = Reference(w, reqs, max_count)
        assert 0 < (ref.verify.status == REFUSED).sum() < nreq // 2
        assert_same(v._result(v.clen, v.content), ref.verify, reqs, f"replay {k}: verify")
        assert_same(e._result(e.plen, e.proofs), ref.extract, reqs, f"replay {k}: extract")
