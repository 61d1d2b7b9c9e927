"""Device-resident slice audits (include/carbonado_hip_audit.h,
carbonado_amd.device extract_slices / verify_slices / verify_slice_proofs):
every request's proof against the host extract_slice, every verdict and every
content byte against the Python oracle's slice verifier (oracle/pyoracle.py:
bao_slice, bao_decode_slice, primed with the clean stream), with every node of
a stream damaged in turn (tests/bao_damage.py).

SIZES are the smallest content lengths at which the tree can go wrong: N = 1
(the chunk is the root: 0, 1, 1023, 1024 bytes), N = 2 with a 1-byte chunk,
N = 3 (odd promotion), 6, 8, 9, 14 with a short last chunk, 24, 66 (more than
one wave of chunks) and 1025.  The streams of a call sit at 56 mod 256 and at
8 mod 256 in one buffer."""
import functools
import random

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from test_slice_verify import _grid
from carbonado_amd import decoding
from carbonado_amd.error import CarbonadoError
from oracle import oracle as O
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 1023, 1024, 1025, 3072, 5121, 8192, 8193, 13317, 24576, 66561, (1 << 20) + 5]
DAMAGE_SIZES = [8192, 13317, 24576, 66561]
GUARD = 4096
MISMATCH = 5


@functools.lru_cache(maxsize=None)
def _stream(n: int):
    """(content, stream, hash) of n seeded bytes; encoded once."""
    d = random.Random(9000 + n).randbytes(n)
    enc, h = O.bao_encode(d)
    return d, enc, h


def _pack_streams(blobs):
    """The streams in one host buffer, alternately at 56 and 8 mod 256."""
    offs, cur = [], 0
    for k, b in enumerate(blobs):
        cur = -(-cur // 256) * 256 + (56 if k % 2 == 0 else 8)
        offs.append(cur)
        cur += len(b)
    host = np.full(cur + 256, 0x5A, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return host, offs


def _untouched(buf: np.ndarray, offs, lens, fill=0xA5) -> bool:
    mask = np.ones(buf.size, dtype=bool)
    for o, n in zip(offs, lens):
        mask[o:o + n] = False
    return bool((buf[mask] == fill).all())


class Call:
    """The device buffers of one batch of requests [(stream, index, count)]
    over `blobs` (streams, content length ns[s] each)."""

    def __init__(self, gpu, blobs, ns, hashes, reqs, align=16):
        import torch
        from carbonado_amd import device as D
        self.torch, self.D, self.L = torch, D, gpu
        self.blobs, self.ns, self.reqs = blobs, ns, reqs
        host, self.in_off = _pack_streams(blobs)
        self.in_len = [len(b) for b in blobs]
        self.streams = torch.from_numpy(host).cuda()
        self.hashes = torch.from_numpy(np.frombuffer(b"".join(hashes) or bytes(32), dtype=np.uint8).copy()).cuda()
        self.hash_list = hashes
        self.rs = [r[0] for r in reqs]
        self.idx = [r[1] for r in reqs]
        self.cnt = [r[2] for r in reqs]
        (self.poff, self.plen, self.coff, self.clen, self.ptotal, self.ctotal) = D.slice_layout(
            [ns[s] for s in self.rs], self.idx, self.cnt, align)
        self.need = gpu.chipa_audit_scratch_len(len(blobs), len(reqs))

    def _scratch(self):
        return self.torch.full((self.need + GUARD,), 0xA5, dtype=self.torch.uint8, device="cuda")

    def extract(self):
        """-> the proofs buffer (device) and every proof's bytes"""
        t = self.torch
        proofs = t.full((self.ptotal + GUARD,), 0xA5, dtype=t.uint8, device="cuda")
        scratch = self._scratch()
        self.D.extract_slices(self.streams, self.in_off, self.in_len, self.rs, self.idx, self.cnt, proofs, self.poff,
                              self.plen, scratch)
        t.cuda.synchronize()
        got = proofs.cpu().numpy()
        assert _untouched(got, self.poff, self.plen), "bytes outside the proof ranges were written"
        assert bool((scratch[self.need:] == 0xA5).all()), "scratch written past chipa_audit_scratch_len"
        return proofs, [got[o:o + n].tobytes() for o, n in zip(self.poff, self.plen)]

    def _verdicts(self, run):
        t = self.torch
        nreq = len(self.reqs)
        content = t.full((self.ctotal + GUARD,), 0xA5, dtype=t.uint8, device="cuda")
        status = t.full((nreq + 8,), -1, dtype=t.int32, device="cuda")
        scratch = self._scratch()
        clen = run(content, status, scratch)
        t.cuda.synchronize()
        assert clen == self.clen
        st = status.cpu().numpy()
        assert bool((st[nreq:] == -1).all()), "status written past nreq"
        assert bool((scratch[self.need:] == 0xA5).all()), "scratch written past chipa_audit_scratch_len"
        return st[:nreq], content.cpu().numpy()

    def verify(self):
        """-> (status per request, the content buffer) straight from the streams"""
        return self._verdicts(lambda content, status, scratch: self.D.verify_slices(
            self.streams, self.in_off, self.in_len, self.hashes, self.rs, self.idx, self.cnt, content, self.coff,
            status, scratch))

    def verify_proofs(self, proofs):
        """-> the same from the proofs buffer alone, one hash per request"""
        t = self.torch
        per_req = b"".join(self.hash_list[s] for s in self.rs) or bytes(32)
        hashes = t.from_numpy(np.frombuffer(per_req, dtype=np.uint8).copy()).cuda()
        return self._verdicts(lambda content, status, scratch: self.D.verify_slice_proofs(
            proofs, self.poff, self.plen, [self.ns[s] for s in self.rs], hashes, self.idx, self.cnt, content,
            self.coff, status, scratch))

    def check(self, got, expected):
        """expected[r] = the request's content, or None where it must fail:
        status, content (zeros where it failed) and the guard bytes around."""
        st, content = got
        want = np.full(content.size, 0xA5, dtype=np.uint8)
        for r, e in enumerate(expected):
            assert st[r] == (0 if e is not None else MISMATCH), (self.reqs[r], st[r])
            assert self.clen[r] == len(e) if e is not None else True, self.reqs[r]
            want[self.coff[r]:self.coff[r] + self.clen[r]] = np.frombuffer(e, dtype=np.uint8) if e is not None else 0
        bad = np.flatnonzero(content != want)
        assert bad.size == 0, f"content differs at byte {bad[:4]} of {content.size}"


def _all_sizes_call(gpu, seed):
    streams = [_stream(n) for n in SIZES]
    reqs = [(s, i, c) for s, n in enumerate(SIZES) for i, c in _grid(n)]
    random.Random(seed).shuffle(reqs)
    return Call(gpu, [e for _, e, _ in streams], SIZES, [h for _, _, h in streams], reqs), streams


def test_extract_equals_the_host_extract_slice(gpu):
    call, streams = _all_sizes_call(gpu, 1)
    assert {o % 256 for o in call.in_off} == {56, 8}
    _, proofs = call.extract()
    for (s, i, c), got in zip(call.reqs, proofs):
        assert got == decoding.extract_slice(streams[s][1], i, c * 1024), (SIZES[s], i, c)


def test_clean_streams_verify_and_return_the_content(gpu):
    call, streams = _all_sizes_call(gpu, 2)
    expected = [streams[s][0][i * 1024:(i + c) * 1024] for s, i, c in call.reqs]
    call.check(call.verify(), expected)
    proofs, _ = call.extract()
    call.check(call.verify_proofs(proofs), expected)


@pytest.mark.parametrize("n", DAMAGE_SIZES)
def test_every_damaged_node_fails_the_requests_that_walk_it(gpu, n):
    """One stream per damaged node (each parent half, each chunk) and the clean
    stream, the full grid of requests on each, all in one call; the verdicts
    are the oracle's slice decoder's."""
    d, enc, h = _stream(n)
    memo = P.bao_prime(enc, h)
    nodes = B.tree_nodes(n)
    rng = random.Random(n)
    blobs = [B.flip(enc, nodes, case, rng) for case in B.every_node_cases(nodes) if nodes[case[0]].size] + [enc]
    grid = _grid(n)
    reqs = [(s, i, c) for s in range(len(blobs)) for i, c in grid]
    expected = []
    for s, i, c in reqs:
        start, length = i * 1024, c * 1024
        try:
            expected.append(P.bao_decode_slice(P.bao_slice(blobs[s], start, length), h, start, length, memo=memo))
        except P.SliceError:
            expected.append(None)
    failed = sum(e is None for e in expected)
    assert 5 * failed >= len(reqs) and 5 * (len(reqs) - failed) >= len(reqs), (failed, len(reqs))
    assert all(e is not None for e in expected[-len(grid):])  # the clean stream, among damaged neighbours
    if n == 66561:
        assert (len(blobs), len(reqs)) == (196 + 1, 12544 + 64)  # every damaged node, and the clean stream
    call = Call(gpu, blobs, [n] * len(blobs), [h] * len(blobs), reqs)
    call.check(call.verify(), expected)
    proofs, _ = call.extract()
    call.check(call.verify_proofs(proofs), expected)


def test_a_bad_header_or_hash_fails_that_stream_alone(gpu):
    ns = [1024, 5121, 13317]
    streams = [_stream(n) for n in ns]
    blobs, hashes, kinds = [], [], []
    for k, (d, enc, h) in enumerate(streams):
        for kind in ("clean", "header", "hash"):
            b, hh = bytearray(enc), bytearray(h)
            if kind == "header":
                b[k % 8] ^= 1 << k
            if kind == "hash":
                hh[5 * k] ^= 0x80
            blobs.append(bytes(b)); hashes.append(bytes(hh)); kinds.append((kind, k))
    reqs = [(s, i, c) for s, (_, k) in enumerate(kinds) for i, c in _grid(ns[k])]
    call = Call(gpu, blobs, [ns[k] for _, k in kinds], hashes, reqs)
    expected = [streams[kinds[s][1]][0][i * 1024:(i + c) * 1024] if kinds[s][0] == "clean" else None
                for s, i, c in reqs]
    call.check(call.verify(), expected)
    proofs, _ = call.extract()
    call.check(call.verify_proofs(proofs), expected)


def test_mixed_call_equals_the_per_request_host_calls(gpu):
    """All sizes, a few requests per stream, two requests with overlapping
    chunk ranges on one stream, some streams damaged; then one request, then
    none.  Every result is the host verify_slice's."""
    rng = random.Random(77)
    blobs, hashes, reqs = [], [], []
    for s, n in enumerate(SIZES):
        d, enc, h = _stream(n)
        if s % 3 == 2:  # damaged somewhere
            nodes = B.tree_nodes(n)
            cases = [c for c in B.every_node_cases(nodes) if nodes[c[0]].size]
            enc = B.flip(enc, nodes, rng.choice(cases), rng)
        blobs.append(enc); hashes.append(h)
        reqs += [(s, i, c) for i, c in rng.sample(_grid(n), min(4, len(_grid(n))))]
    big = SIZES.index(66561)
    reqs += [(big, 3, 40), (big, 20, 30)]  # chunks [3, 43) and [20, 50) of one stream
    rng.shuffle(reqs)

    def host(s, i, c):
        try:
            return decoding.verify_slice(hashes[s], blobs[s], i, c)
        except CarbonadoError:
            return None

    expected = [host(*r) for r in reqs]
    assert any(e is None for e in expected) and any(e for e in expected)
    call = Call(gpu, blobs, SIZES, hashes, reqs, align=256)
    call.check(call.verify(), expected)
    proofs, _ = call.extract()
    call.check(call.verify_proofs(proofs), expected)
    one = Call(gpu, blobs, SIZES, hashes, [(big, 20, 30)])
    one.check(one.verify(), [host(big, 20, 30)])
    none = Call(gpu, blobs, SIZES, hashes, [])
    none.check(none.verify(), [])
    proofs, got = none.extract()
    assert got == []
    none.check(none.verify_proofs(proofs), [])
