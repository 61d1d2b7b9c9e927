"""The device calls at offsets and pitches of 2^32 and more (tests/far_world.py).

Every family that carries 64-bit offsets to the device in a table and does the
address arithmetic in a kernel is run once with what it reads and what it
writes placed across byte 2^32 of a flat buffer: the compact world its own
module builds, moved to BASE(cut), with one named object or stream containing
bytes 2^32 - 1 and 2^32, something entirely below and something entirely
above.  The expected bytes are the ones the family's module compares with (the
CPU oracle, EVP, the Python slice verifier, the objects' bytes, the
host-planned call), never a second run of the call at low offsets.

An offset that lost its upper bits does not fault; it reads another stream's
bytes or writes 4 GiB lower.  The first shows as a miscompare, the second is
caught by Far.untouched_outside(): every byte of both buffers outside the
windows a call may write still holds the canary.

The two buffers (what a call reads, what it writes) are 2^32 + 64 MiB each and
live for this module only."""
import numpy as np
import pytest

import far_world as FW  # tests/far_world.py (tests/ is on sys.path under pytest)
import read_world as RW
from far_world import BASE, CANARY, FOUR_GIB, assert_straddles, cut_for

pytestmark = pytest.mark.gpu

ROOM = 64 << 20
GUARD = 4096
FAR_PITCH = FOUR_GIB + 256


@pytest.fixture(scope="module")
def far(gpu):
    import torch
    pair = [FW.Far(ROOM), FW.Far(ROOM)]
    yield pair
    for f in pair:
        f.buf = None
    pair.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _canary_back(far):
    yield
    for f in far:
        f.reset()


def _shifted(base, offs):
    return [base + o for o in offs]


def _same(got: np.ndarray, want: np.ndarray, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: first differing byte at {bad[:4]} of {got.size}"


def _guarded(image: np.ndarray, guard=GUARD) -> np.ndarray:
    """the compact image with `guard` canary bytes on each side: what Far.window(base, size, guard) must hold"""
    out = np.full(image.size + 2 * guard, CANARY, dtype=np.uint8)
    out[guard:guard + image.size] = image
    return out


def _only_written(f: FW.Far, windows):
    ok = f.untouched_outside(windows)
    assert ok, f"a byte outside the call's ranges was written, the first at {f.first_touched(windows)}"


def _clean(f: FW.Far, base, size):
    """after a test: the window it used and the low region a narrowed offset would have hit"""
    f.refill([(base - GUARD, size + 2 * GUARD)], low=size + GUARD)


# ---- ragged encode / decode at 4, 8, 12 -------------------------------------------------
RAGGED_SIZES = [1, 4097, 300001, 65537]   # 300001: several 64-chunk groups, so group and top kernels on both sides
RAGGED_NAMED = 2


def _ragged_cut(level, off, length):
    """Half way into the named range; at level 8 (eight shards and nothing
    else) half way is a shard's first byte, so the boundary is moved on by half
    a shard to fall inside one."""
    skew = 0 if level & 4 else (length // 8 // 2) // 256 * 256
    return cut_for(off, length) + skew


@pytest.mark.parametrize("level", [4, 8, 12])
def test_ragged_encode_and_decode(gpu, far, level):
    import torch
    from carbonado_amd import device as D
    import test_gpu_ragged as TR
    src, dst = far
    sizes, named = RAGGED_SIZES, RAGGED_NAMED
    plain, p_off = TR._pack([TR._data(n) for n in sizes], fill=0x5A)
    s_off, s_len, s_total = D.ragged_layout(level, sizes, align=256, stream_offset=56)
    oracle = [TR._oracle(n, level) for n in sizes]
    assert [len(e) for e, _, _ in oracle] == s_len
    streams = np.full(s_total, 0x5A, dtype=np.uint8)
    for o, (enc, _, _) in zip(s_off, oracle):
        streams[o:o + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    p_base = BASE(cut_for(p_off[named], sizes[named]))
    s_base = BASE(_ragged_cut(level, s_off[named], s_len[named]))
    assert_straddles(p_base, p_off, sizes, named)
    assert_straddles(s_base, s_off, s_len, named)
    if level == 8:  # the boundary inside a shard
        C = s_len[named] // 8
        assert (FOUR_GIB - (s_base + s_off[named])) % C >= 1024

    # encode: plaintexts far in src, streams far in dst
    src.put(plain, p_base)
    hashes = torch.full((len(sizes), 32), 0xA5, dtype=torch.uint8, device="cuda")
    out_len, infos = D.encode_ragged(level, src.buf, _shifted(p_base, p_off), sizes, dst.buf, _shifted(s_base, s_off),
                                     hashes, D.ragged_scratch(level, sizes))
    torch.cuda.synchronize()
    assert out_len == s_len
    want = streams.copy()
    keep = np.ones(s_total, dtype=bool)
    for o, n in zip(s_off, s_len):
        keep[o:o + n] = False
    want[keep] = CANARY
    _same(dst.window(s_base, s_total, GUARD), _guarded(want), ("encode", level))
    gh = hashes.cpu().numpy()
    for i, (_, h, info) in enumerate(oracle):
        assert gh[i].tobytes() == h, (level, sizes[i])
        TR._check_info(infos[i], info, (level, sizes[i]))
    _only_written(dst, [(s_base, s_total)])
    _only_written(src, [(p_base, plain.size)])
    _same(src.window(p_base, plain.size), plain, "the input changed")
    _clean(dst, s_base, s_total)
    _clean(src, p_base, plain.size)

    # decode: the oracle's streams far in src, content far in dst
    src.put(streams, s_base)
    hashes = torch.from_numpy(np.frombuffer(b"".join(h for _, h, _ in oracle), dtype=np.uint8).copy()).cuda()
    padding = [info["padding_len"] for _, _, info in oracle]
    status = torch.full((len(sizes),), 77, dtype=torch.int32, device="cuda")
    exp, _ = TR._pack([TR._data(n) for n in sizes], fill=CANARY)
    dec_len = D.decode_ragged(level, src.buf, _shifted(s_base, s_off), s_len, hashes, padding, dst.buf,
                              _shifted(p_base, p_off), status, D.ragged_scratch(level, s_len, decode=True))
    torch.cuda.synchronize()
    assert dec_len == list(sizes) and status.cpu().tolist() == [0] * len(sizes)
    _same(dst.window(p_base, exp.size, GUARD), _guarded(exp), ("decode", level))
    _only_written(dst, [(p_base, exp.size)])
    _only_written(src, [(s_base, s_total)])
    _clean(dst, p_base, exp.size)
    _clean(src, s_base, s_total)


# ---- AES-256-GCM over ragged messages ---------------------------------------------------
GCM_LENS = [0, 1, 17, 8191, 8193, 64 * 8192 + 1, 2 * 8192 + 1]   # 64 items + 1: a second-level step on both sides
GCM_NAMED = 5


def test_gcm_seal_and_open(gpu, far):
    import torch
    from carbonado_amd import device as D
    import test_gpu_ecies_dev as TE
    src, dst = far
    b = TE.Batch(GCM_LENS, seed=31)
    named = GCM_NAMED
    p_base = BASE(cut_for(b.in_off[named], b.lens[named]))
    c_base = BASE(cut_for(b.out_off[named], b.lens[named]))
    for base, offs in ((p_base, b.in_off), (c_base, b.out_off)):
        lens = [max(n, 1) for n in b.lens]  # an empty message lies where its offset lies
        assert_straddles(base, offs, lens, named)
    assert len({o % 16 for o in b.out_off}) >= 6  # the ciphertexts at several residues, as Batch places them

    src.put(b.plain_image(0x11), p_base)
    tags = torch.full((16 * b.count + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    D.gcm_seal_ragged(b.keys, b.ivs, src.buf, _shifted(p_base, b.in_off), b.lens, dst.buf, _shifted(c_base, b.out_off),
                      tags, D.gcm_scratch(b.lens))
    torch.cuda.synchronize()
    assert bytes(tags.cpu().numpy()) == b"".join(b.tags) + b"\xA5" * 16
    _same(dst.window(c_base, b.out_size, GUARD), _guarded(b.cipher_image(CANARY)), "seal")
    _only_written(dst, [(c_base, b.out_size)])
    _only_written(src, [(p_base, b.in_size)])
    _clean(dst, c_base, b.out_size)
    _clean(src, p_base, b.in_size)

    src.put(b.cipher_image(0x3C), c_base)
    status = torch.full((b.count + 1,), 0x7777, dtype=torch.int32, device="cuda")
    D.gcm_open_ragged(b.keys, b.ivs, src.buf, _shifted(c_base, b.out_off), b.lens,
                      RW.dev(np.frombuffer(b"".join(b.tags), dtype=np.uint8)), dst.buf, _shifted(p_base, b.in_off),
                      status, D.gcm_scratch(b.lens))
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[:b.count] == 0).all() and st[b.count] == 0x7777
    _same(dst.window(p_base, b.in_size, GUARD), _guarded(b.plain_image(CANARY)), "open")
    _only_written(dst, [(p_base, b.in_size)])
    _only_written(src, [(c_base, b.out_size)])
    _clean(dst, p_base, b.in_size)
    _clean(src, c_base, b.out_size)


# ---- the keystream over ranges (in place) -----------------------------------------------
def test_keystream_over_ranges(gpu, far):
    import torch
    from carbonado_amd import device as D
    import test_gpu_cread as TC
    _, dst = far
    it = TC._raw_items()
    named = it.n.index(2 * TC.UNIT_SPAN + 1)
    base = BASE(cut_for(it.off[named], it.n[named]))
    assert_straddles(base, it.off, [max(n, 1) for n in it.n], named)
    dst.put(it.image(it.ct), base)
    D.ctr_ranges(it.keys, it.ivs, it.key, it.pos, it.n, dst.buf, _shifted(base, it.off), D.ctr_scratch(3, len(it.n)))
    torch.cuda.synchronize()
    _same(dst.window(base, it.size, GUARD), _guarded(it.image(it.pt)), "keystream")
    _only_written(dst, [(base, it.size)])
    _clean(dst, base, it.size)


# ---- ranged reads: host-planned and device-planned --------------------------------------
READ_NAMED = 5   # the stream of shard length 65536


class FarReadWorld:
    """test_gpu_qread's World with its streams moved across 2^32 of `f`: the
    same hashes, paddings and shard lengths, off = base + the compact offsets,
    and a stream table over those."""

    def __init__(self, w, f: FW.Far):
        self.torch, self.D, self.low = w.torch, w.D, w
        self.size = w.buf.numel()
        self.base = BASE(cut_for(w.off[READ_NAMED], w.len[READ_NAMED]))
        assert_straddles(self.base, w.off, w.len, READ_NAMED)
        f.put(w.buf, self.base)
        self.buf, self.off, self.len = f.buf, _shifted(self.base, w.off), w.len
        self.hashes, self.pads, self.cls, self.objects = w.hashes, w.pads, w.cls, w.objects
        self.table = w.D.stream_table(self.buf, self.off, self.len, self.hashes, self.pads, self.cls)
        w.torch.cuda.synchronize()
        assert (self.table.nstreams, self.table.max_chunks, self.table.min_shard) == (len(w.off), 512, 1024)


def _content_named(reqs, max_len):
    """the request whose content slot is put across 2^32: max_len bytes from inside the named stream"""
    return reqs.index((READ_NAMED, 65536 - 2000, max_len, 0))


def test_host_planned_reads(gpu, far):
    """read_ranges and read_ranges_vouched: the base set of test_gpu_qread over
    the far streams into far content, held to what that module pins for them
    (the clean objects' bytes, every damage class and its status)."""
    import test_gpu_qread as TQ
    src, dst = far
    fw = FarReadWorld(TQ.world(), src)
    max_len = 4096
    stride = RW.up16(max_len) + 16
    reqs = TQ.base_requests(max_len)
    named = _content_named(reqs, max_len)
    c_base = BASE(cut_for(named * stride, max_len))
    size = len(reqs) * stride + 64
    assert_straddles(c_base, [r * stride for r in range(len(reqs))], [stride - 16] * len(reqs), named)
    calls = []

    def reference(w, rq, ml, st, vouched, flags=0):
        assert (ml, st) == (max_len, stride)
        got = TQ.reference(w, rq, ml, st, vouched, flags, content=dst.buf, content_base=c_base)
        assert got.clen[named] == max_len
        _only_written(dst, [(c_base + r * stride, n) for r, n in enumerate(got.clen)])
        dst.refill([(c_base, size)])
        calls.append(vouched)
        return got

    TQ.check_base_set(fw, reference, max_lens=(max_len,))
    assert calls.count(True) == 2 and calls.count(False) == 1
    _only_written(src, [(fw.base, fw.size)])
    _same(src.window(fw.base, fw.size), fw.low.host, "a read changed the streams")
    _clean(dst, c_base, size)
    _clean(src, fw.base, fw.size)


class FarPlanned:
    """A read_world.Planned (p) with its content slots in a far buffer: slot r
    at base + r * pitch of f.  The content comes back as the compact image of
    the family's module (slot r at r * stride), so its comparison serves as it is."""

    def __init__(self, p: RW.Planned, f: FW.Far, base, pitch):
        self.p = p
        self.f, self.base, self.pitch, self.compact = f, base, pitch, self.p.stride
        self.p.content, self.p.stride = f.buf[base:], pitch

    def slots(self, lens):
        return [(self.base + r * self.pitch, n) for r, n in enumerate(lens)]

    def run(self, reqs, flags=0) -> RW.Got:
        p, torch, n = self.p, self.p.w.torch, self.p.nreq
        p.rs.copy_(torch.tensor([r[0] for r in reqs], dtype=torch.int32))
        p.start.copy_(torch.tensor([r[1] for r in reqs], dtype=torch.int64))
        p.length.copy_(torch.tensor([r[2] for r in reqs], dtype=torch.int64))
        p.enqueue(flags)
        torch.cuda.synchronize()
        assert (p.full[p.scratch.numel():] == RW.GUARD).all().item(), "bytes behind scratch_len were written"
        assert (p.status[n:] == 0x5A5A5A5A).all().item() and (p.used[n:] == 0x3C3C3C3C).all().item()
        assert (p.vouch[n if p.vouched else 0:] == 0x69696969).all().item()
        clen = p.clen.cpu().numpy().tolist()
        content = np.full(n * self.compact + 64, CANARY, dtype=np.uint8)
        for r, (at, _) in enumerate(self.slots(clen)):
            content[r * self.compact:(r + 1) * self.compact] = self.f.window(at, self.compact)
        _only_written(self.f, self.slots(clen))
        self.f.refill(self.slots([self.compact] * n))
        return RW.Got(p.status[:n].cpu().numpy(), p.used[:n].cpu().numpy(),
                      p.vouch[:n].cpu().numpy() if p.vouched else None, clen, content)


def test_device_planned_reads(gpu, far):
    """read_ranges_planned and read_ranges_vouched_planned over a stream table
    of far offsets into far content, against the host-planned calls as
    test_gpu_qread compares them."""
    import test_gpu_qread as TQ
    src, dst = far
    w = TQ.world()
    fw = FarReadWorld(w, src)
    max_len = 4096
    reqs = TQ.base_requests(max_len)
    nreq, stride = len(reqs), RW.up16(max_len) + 16
    named = _content_named(reqs, max_len)
    c_base = BASE(cut_for(named * stride, max_len))
    assert_straddles(c_base, [r * stride for r in range(nreq)], [stride - 16] * nreq, named)
    for vouched, flags in ((False, 0), (True, 0), (True, w.D.VREAD_STRICT)):
        got = FarPlanned(TQ.Planned(fw, nreq, max_len, vouched), dst, c_base, stride).run(reqs, flags)
        assert got.clen[named] == max_len
        RW.assert_equal(got, TQ.reference(w, reqs, max_len, stride, vouched, flags), reqs)
    _only_written(src, [(fw.base, fw.size)])
    _same(src.window(fw.base, fw.size), w.host, "a read changed the streams")
    _clean(dst, c_base, nreq * stride + 64)
    _clean(src, fw.base, fw.size)


def test_planned_reads_content_stride_past_4gib(gpu, far):
    """Two requests, content_stride 2^32 + 256: slot 0 at byte 0, slot 1 past the boundary."""
    import test_gpu_qread as TQ
    _, dst = far
    w = TQ.world()
    max_len = 4096
    reqs = [(5, 65536 - 2000, max_len, 0), (3, 1000, 3000, 0)]
    stride = RW.up16(max_len) + 16
    for vouched in (False, True):
        fp = FarPlanned(TQ.Planned(w, 2, max_len, vouched), dst, 0, FAR_PITCH)
        got = fp.run(reqs)
        assert got.clen == [max_len, 3000] and got.status.tolist() == [0, 0]
        for r, (s, a, n, _) in enumerate(reqs):  # both slots hold the objects' bytes
            _same(got.content[r * stride:r * stride + n], w.objects[s][a:a + n], ("slot", r))
        RW.assert_equal(got, TQ.reference(w, reqs, max_len, stride, vouched), reqs)
    dst.refill([], low=stride + GUARD)


# ---- slice audits -----------------------------------------------------------------------
AUDIT_SIZES = [1, 70001, 5121]
AUDIT_NAMED = 1


def test_slice_audits(gpu, far):
    """extract_slices, verify_slices and verify_slice_proofs of level-4 streams:
    streams, proofs and content each across 2^32, against the Python oracle's
    bao_slice / bao_decode_slice."""
    import torch
    from carbonado_amd import device as D
    from oracle import pyoracle as P
    import test_gpu_audit as TA
    from test_slice_verify import _grid
    src, dst = far
    made = [TA._stream(n) for n in AUDIT_SIZES]
    blobs, hash_list = [e for _, e, _ in made], [h for _, _, h in made]
    host, in_off = TA._pack_streams(blobs)
    in_len = [len(b) for b in blobs]
    reqs = [(s, i, c) for s, n in enumerate(AUDIT_SIZES) for i, c in _grid(n)]
    rs, idx, cnt = ([r[k] for r in reqs] for k in range(3))
    poff, plen, coff, clen, ptotal, ctotal = D.slice_layout([AUDIT_SIZES[s] for s in rs], idx, cnt, 16)
    N = -(-AUDIT_SIZES[AUDIT_NAMED] // 1024)
    named = reqs.index((AUDIT_NAMED, 0, N))  # the whole of the 70001 stream: the largest proof and content
    memo = [P.bao_prime(e, h) for e, h in zip(blobs, hash_list)]
    want_proof = [P.bao_slice(blobs[s], i * 1024, c * 1024) for s, i, c in reqs]
    want_content = [P.bao_decode_slice(want_proof[r], hash_list[s], i * 1024, c * 1024, memo=memo[s])
                    for r, (s, i, c) in enumerate(reqs)]
    assert [len(p) for p in want_proof] == plen and [len(c) for c in want_content] == clen
    s_base = BASE(cut_for(in_off[AUDIT_NAMED], in_len[AUDIT_NAMED]))
    p_base = BASE(cut_for(poff[named], plen[named]))
    c_base = BASE(cut_for(coff[named], clen[named]))
    assert_straddles(s_base, in_off, in_len, AUDIT_NAMED)
    # ranges of the layouts may be empty; the named ones are not, and only they lie across
    assert_straddles(p_base, poff, [max(n, 1) for n in plen], named)
    assert_straddles(c_base, coff, [max(n, 1) for n in clen], named)
    hashes = RW.dev(np.frombuffer(b"".join(hash_list), dtype=np.uint8))
    per_req = RW.dev(np.frombuffer(b"".join(hash_list[s] for s in rs), dtype=np.uint8))
    proof_image = np.full(ptotal, CANARY, dtype=np.uint8)
    for o, p in zip(poff, want_proof):
        proof_image[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    content_image = np.full(ctotal, CANARY, dtype=np.uint8)
    for o, c in zip(coff, want_content):
        content_image[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)

    src.put(host, s_base)
    D.extract_slices(src.buf, _shifted(s_base, in_off), in_len, rs, idx, cnt, dst.buf, _shifted(p_base, poff), plen,
                     D.audit_scratch(len(blobs), len(reqs)))
    torch.cuda.synchronize()
    _same(dst.window(p_base, ptotal, GUARD), _guarded(proof_image), "extract_slices")
    _only_written(dst, [(p_base, ptotal)])
    _clean(dst, p_base, ptotal)

    status = torch.full((len(reqs) + 8,), -1, dtype=torch.int32, device="cuda")
    got_len = D.verify_slices(src.buf, _shifted(s_base, in_off), in_len, hashes, rs, idx, cnt, dst.buf,
                              _shifted(c_base, coff), status, D.audit_scratch(len(blobs), len(reqs)))
    torch.cuda.synchronize()
    assert got_len == clen and status.cpu().tolist() == [0] * len(reqs) + [-1] * 8
    _same(dst.window(c_base, ctotal, GUARD), _guarded(content_image), "verify_slices")
    _only_written(dst, [(c_base, ctotal)])
    _only_written(src, [(s_base, host.size)])
    _clean(dst, c_base, ctotal)
    _clean(src, s_base, host.size)

    src.put(proof_image, p_base)  # the oracle's proofs, far
    status.fill_(-1)
    got_len = D.verify_slice_proofs(src.buf, _shifted(p_base, poff), plen, [AUDIT_SIZES[s] for s in rs], per_req, idx,
                                    cnt, dst.buf, _shifted(c_base, coff), status, D.audit_scratch(len(reqs), len(reqs)))
    torch.cuda.synchronize()
    assert got_len == clen and status.cpu().tolist() == [0] * len(reqs) + [-1] * 8
    _same(dst.window(c_base, ctotal, GUARD), _guarded(content_image), "verify_slice_proofs")
    _only_written(dst, [(c_base, ctotal)])
    _only_written(src, [(p_base, ptotal)])
    _clean(dst, c_base, ctotal)
    _clean(src, p_base, ptotal)


# ---- ragged scrub and shard masks -------------------------------------------------------
SCRUB_NAMED = 2


def _scrub_objects():
    """Four streams of spc 1, 3, 13, 13 with the damage kinds of
    test_gpu_scrub_ragged: a chunk of one shard, the root (unrepairable), a
    chunk in each of shards 1 and 6 of the named stream, and none."""
    import random
    import bao_damage as B
    import test_gpu_scrub_ragged as TS

    def chunk_of(spc, shard, rng):
        leaves = [k for k, nd in enumerate(B.tree_nodes(8192 * spc)) if not nd.parent]
        return leaves[shard * spc + rng.randrange(spc)], -1

    rng = random.Random("far scrub")
    return [TS._obj(1, ("far", 0), [chunk_of(1, 2, rng)], rng, "shard 2"),
            TS._obj(3, ("far", 1), [(0, rng.randrange(2))], rng, "root"),
            TS._obj(13, ("far", 2), [chunk_of(13, 1, rng), chunk_of(13, 6, rng)], rng, "shards 1 and 6"),
            TS._obj(13, ("far", 3), [], rng, "none")]


def test_scrub_ragged_and_shard_masks(gpu, far):
    import torch
    from carbonado_amd import device as D
    import test_gpu_scrub_ragged as TS
    src, dst = far
    objs = _scrub_objects()
    named = SCRUB_NAMED
    assert [o.spc for o in objs] == [1, 3, 13, 13] and [o.status for o in objs] == [0, 7, 0, 12]
    assert sorted(set(range(8)) - objs[named].good) == [1, 6]
    host, off, total = TS._input(objs)
    in_len = [len(o.clean) for o in objs]
    base = BASE(cut_for(off[named], in_len[named]))
    assert_straddles(base, off, in_len, named)
    (lo, _), (hi, _) = sorted(objs[named].flips)  # one damaged shard on each side of 2^32
    assert base + off[named] + lo < FOUR_GIB <= base + off[named] + hi
    src.put(host, base)
    far_off = _shifted(base, off)
    hashes = TS._hashes(objs)
    pads, cls = [o.padding for o in objs], [o.chunk_len for o in objs]

    masks = torch.full((len(objs) + 8,), -1, dtype=torch.int32, device="cuda")
    D.shard_masks_ragged(src.buf, far_off, in_len, hashes, cls, D.scrub_ragged_scratch(in_len, 1), masks=masks)
    torch.cuda.synchronize()
    assert masks.tolist() == [o.mask for o in objs] + [-1] * 8

    status = D.scrub_ragged(src.buf, far_off, in_len, hashes, pads, cls, dst.buf, far_off,
                            D.scrub_ragged_scratch(in_len))
    torch.cuda.synchronize()
    assert status.tolist() == [o.status for o in objs]
    want = np.full(total, CANARY, dtype=np.uint8)
    for j, o in enumerate(objs):
        if o.status == 0:
            want[off[j]:off[j] + in_len[j]] = np.frombuffer(o.clean, dtype=np.uint8)
    _same(dst.window(base, total, GUARD), _guarded(want), "scrub_ragged")
    _only_written(dst, [(base, total)])
    _only_written(src, [(base, total)])
    _same(src.window(base, total), host, "scrub_ragged changed its input")

    # in place: the repaired streams are clean where they lie, the others as they were
    status = D.scrub_ragged(src.buf, far_off, in_len, hashes, pads, cls, src.buf, far_off,
                            D.scrub_ragged_scratch(in_len))
    torch.cuda.synchronize()
    assert status.tolist() == [o.status for o in objs]
    want = host.copy()
    for j, o in enumerate(objs):
        if o.status == 0:
            want[off[j]:off[j] + in_len[j]] = np.frombuffer(o.clean, dtype=np.uint8)
    _same(src.window(base, total, GUARD), _guarded(want), "scrub_ragged in place")
    _only_written(src, [(base, total)])
    _clean(dst, base, total)
    _clean(src, base, total)


# ---- Ecies envelopes, host-made and device-made keys ------------------------------------
def test_ecies_envelopes(gpu, far):
    """ecies_seal_ragged / ecies_open_ragged and their _dev_keys forms over the
    envelopes of test_gpu_agree, against the Python oracle's ecies_encrypt."""
    import torch
    from carbonado_amd import device as D
    from oracle import host_oracle as H
    import test_gpu_agree as TG
    from test_gpu_ecies_dev import SECRET, Envelopes
    src, dst = far
    e = Envelopes(TG.ENV_LENS, seed=29, residues=(0, 3, 8, 15))
    named = e.lens.index(8193)
    env_len = [n + 97 for n in e.lens]
    p_base = BASE(cut_for(e.in_off[named], e.lens[named]))
    e_base = BASE(cut_for(e.env_off[named], env_len[named]))
    assert_straddles(p_base, e.in_off, [max(n, 1) for n in e.lens], named)
    assert_straddles(e_base, e.env_off, env_len, named)
    py = [H.ecies_encrypt(e.pub, p, sk, nonce) for p, (sk, nonce) in zip(e.pt, e.inject)]
    sealed = e.env_image(CANARY, envs=py)
    seals = ((D.ecies_seal_ragged, D.gcm_scratch), (D.ecies_seal_ragged_dev_keys, D.envelope_scratch))
    opens = ((D.ecies_open_ragged, D.gcm_scratch), (D.ecies_open_ragged_dev_keys, D.envelope_scratch))

    src.put(e.plain_image(0x11), p_base)
    for call, scratch in seals:
        call(e.pub, src.buf, _shifted(p_base, e.in_off), e.lens, dst.buf, _shifted(e_base, e.env_off), scratch(e.lens),
             inject=e.inject)
        torch.cuda.synchronize()
        _same(dst.window(e_base, e.env_size, GUARD), _guarded(sealed), call.__name__)
        _only_written(dst, [(e_base, e.env_size)])
        _only_written(src, [(p_base, e.in_size)])
        _clean(dst, e_base, e.env_size)
    _clean(src, p_base, e.in_size)

    src.put(e.env_image(0x3C, envs=py), e_base)
    for call, scratch in opens:
        status = torch.full((e.count,), 0x7777, dtype=torch.int32, device="cuda")
        olen = call(SECRET, src.buf, _shifted(e_base, e.env_off), env_len, dst.buf, _shifted(p_base, e.in_off), status,
                    scratch(e.lens))
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * e.count and olen == e.lens
        _same(dst.window(p_base, e.in_size, GUARD), _guarded(e.plain_image(CANARY)), call.__name__)
        _only_written(dst, [(p_base, e.in_size)])
        _only_written(src, [(e_base, e.env_size)])
        _clean(dst, p_base, e.in_size)
    _clean(src, e_base, e.env_size)


ECIES_SIZES = [0, 1, 927, 5000, 4096 - 97]   # SIZES of test_gpu_agree without the 1 MiB object; 5000 not last
ECIES_NAMED = 3


def test_ecies_one_call_forms_at_13(gpu, far):
    """encode_ragged_ecies / decode_ragged_ecies and their _dev_keys forms at
    level 13, against the C oracle's encode with the same injected values."""
    import torch
    from carbonado_amd import device as D
    from oracle import oracle as O
    import test_gpu_agree as TG
    from test_gpu_ecies_dev import SECRET, Objects, _same_info
    src, dst = far
    assert sorted(ECIES_SIZES) == sorted(n for n in TG.SIZES if n != 1 << 20)
    s = Objects(13, ECIES_SIZES, seed=66)
    named = ECIES_NAMED
    want = [O.c_encode_full(s.pt[o], 13, s.pub, *s.inject[o]) for o in range(s.count)]
    s_len = [len(enc) for enc, _, _ in want]
    assert s_len == s.need
    streams = np.full(s.total + 64, CANARY, dtype=np.uint8)
    for o, (enc, _, _) in enumerate(want):
        streams[s.out_off[o]:s.out_off[o] + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    p_base = BASE(cut_for(s.in_off[named], s.lens[named]))
    s_base = BASE(cut_for(s.out_off[named], s_len[named]))
    assert_straddles(p_base, s.in_off, [max(n, 1) for n in s.lens], named)
    assert_straddles(s_base, s.out_off, s_len, named)
    encodes = ((D.encode_ragged_ecies, D.ecies_ragged_scratch), (D.encode_ragged_ecies_dev_keys, D.ecies_ragged_scratch_dev_keys))
    decodes = ((D.decode_ragged_ecies, D.ecies_ragged_scratch), (D.decode_ragged_ecies_dev_keys, D.ecies_ragged_scratch_dev_keys))

    src.put(s.plain_image(0x11), p_base)
    for call, scratch in encodes:
        hashes = torch.full((s.count, 32), 0xEE, dtype=torch.uint8, device="cuda")
        olen, info = call(13, s.pub, src.buf, _shifted(p_base, s.in_off), s.lens, dst.buf, _shifted(s_base, s.out_off),
                          hashes, scratch(13, s.lens), inject=s.inject)
        torch.cuda.synchronize()
        assert olen == s_len
        _same(dst.window(s_base, streams.size, GUARD), _guarded(streams), call.__name__)
        hh = hashes.cpu().numpy()
        for o, (_, h, winfo) in enumerate(want):
            assert bytes(hh[o]) == h, o
            _same_info(info[o], winfo)
        _only_written(dst, [(s_base, streams.size)])
        _only_written(src, [(p_base, s.in_size)])
        _clean(dst, s_base, streams.size)
    _clean(src, p_base, s.in_size)

    src.put(streams, s_base)
    hashes = RW.dev(np.frombuffer(b"".join(h for _, h, _ in want), dtype=np.uint8)).view(s.count, 32)
    pads = [winfo["padding_len"] for _, _, winfo in want]
    for call, scratch in decodes:
        status = torch.full((s.count,), 0x7777, dtype=torch.int32, device="cuda")
        plen = call(13, SECRET, src.buf, _shifted(s_base, s.out_off), s_len, hashes, pads, dst.buf,
                    _shifted(p_base, s.in_off), status, scratch(13, s_len, decode=True))
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * s.count and plen == s.lens
        _same(dst.window(p_base, s.in_size, GUARD), _guarded(s.plain_image(CANARY)), call.__name__)
        _only_written(dst, [(p_base, s.in_size)])
        _only_written(src, [(s_base, streams.size)])
        _clean(dst, p_base, s.in_size)
    _clean(src, s_base, streams.size)


def test_key_agreement_pitches_at_and_past_4gib(gpu, far):
    """seal_keys and open_keys refuse a pitch above 2^32 on purpose
    (include/carbonado_hip_agree.h: INVALID_ARG, nothing enqueued): pinned for
    every pitch at 2^32 + 256.  At the largest pitch they take, 2^32, entry 1
    lies at byte 2^32: two entries with injected secrets against the Python
    oracle's secp256k1 and HKDF."""
    import torch
    from carbonado_amd import device as D
    from carbonado_amd.error import InvalidArgument
    from oracle import host_oracle as H
    from test_gpu_ecies_dev import SECRET
    src, dst = far
    ks = [H.N - 1, 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211122334455667788 % H.N]
    sk = b"".join(k.to_bytes(32, "big") for k in ks)
    receiver = H.public_key(SECRET)
    peer = H.parse_pubkey(receiver)
    pub = [H.ser_uncompressed(H.point_mul(k)) for k in ks]
    keys = [H.hkdf_sha256(e + H.ser_uncompressed(H.point_mul(k, peer))) for e, k in zip(pub, ks)]
    status = torch.full((4,), 0x7777, dtype=torch.int32, device="cuda")

    for pitches in ((FAR_PITCH, 32), (65, FAR_PITCH), (FAR_PITCH, FAR_PITCH)):
        with pytest.raises(InvalidArgument):
            D.seal_keys(receiver, 2, dst.buf, pitches[0], src.buf, pitches[1], D.agree_scratch(2), eph_sk=sk)
        with pytest.raises(InvalidArgument):
            D.open_keys(SECRET, src.buf, pitches[0], 2, dst.buf, pitches[1], status, D.agree_scratch(2))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0x7777] * 4
    _only_written(dst, [])
    _only_written(src, [])

    pitch = FOUR_GIB
    slot = [0, pitch]

    def holds(f, rows, what):
        for at, r in zip(slot, rows):
            _same(f.window(at, len(r)), np.frombuffer(r, dtype=np.uint8), (what, at))
        _only_written(f, [(at, len(r)) for at, r in zip(slot, rows)])

    D.seal_keys(receiver, 2, dst.buf, pitch, src.buf, pitch, D.agree_scratch(2), eph_sk=sk)
    torch.cuda.synchronize()
    holds(dst, pub, "seal_keys pub")
    holds(src, keys, "seal_keys keys")
    for f in (src, dst):
        f.refill([(at, 256) for at in slot])

    for at, r in zip(slot, pub):
        src.put(np.frombuffer(r, dtype=np.uint8), at)
    D.open_keys(SECRET, src.buf, pitch, 2, dst.buf, pitch, status, D.agree_scratch(2))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0x7777, 0x7777]
    holds(dst, keys, "open_keys keys")
    holds(src, pub, "open_keys changed the ephemeral keys")
    for f in (src, dst):
        f.refill([(at, 256) for at in slot])


# ---- plaintext reads of level-13 streams, and the key table made on the device ----------
PLAIN_SIZES = [1, 927, 2000, 70000, 3999, 100, 3000]
PLAIN_NAMED, PLAIN_SMALL = 3, 4
PLAIN_SO = 16    # chunk 0 of an 8-chunk stream then starts at 216 mod 256: its first 81 bytes contain a multiple of 256
PLAIN_SECRET = bytes(range(1, 33))


class PlainWorld(RW.PlainStreams):
    """Seven level-13 streams made on the device at low offsets, one chunk of
    primary shard 1 of the 70000-byte one damaged (its reads are rebuilt from
    the shards on the other side of 2^32), and their host-made keys."""

    def __init__(self):
        import torch
        import bao_damage as B
        from carbonado_amd import device as D
        from oracle import oracle as O
        self.torch, self.D = torch, D
        rng = np.random.default_rng(71)
        sizes, self.count = PLAIN_SIZES, len(PLAIN_SIZES)
        self.pt = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
        inject = [(rng.integers(1, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
                  for _ in sizes]
        in_off, plain = self.place_plain(sizes)
        self.off, _, total = D.ragged_layout(12, [n + 97 for n in sizes], 256, PLAIN_SO)
        buf = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((self.count, 32), dtype=torch.uint8, device="cuda")
        self.len, info = D.encode_ragged_ecies(13, O.c_public_key(PLAIN_SECRET), RW.dev(plain), in_off, sizes, buf, self.off,
                                               self.hashes, D.ecies_ragged_scratch(13, sizes), inject=inject)
        self.pads, self.cls = [i.padding_len for i in info], [i.chunk_len for i in info]
        assert self.cls[PLAIN_SMALL] == 1024 and self.cls[PLAIN_NAMED] == 18 * 1024
        spc = self.cls[PLAIN_NAMED] // 1024
        self.damaged = (1, 2)  # (shard, chunk in it)
        buf[self.off[PLAIN_NAMED] + B.chunk_offsets(spc)[spc * 1 + 2] + 300] ^= 0x10
        self.keys, self.ivs, self.kstat = D.stream_keys(PLAIN_SECRET, buf, self.off, self.len, self.hashes, self.pads,
                                                        self.cls, D.stream_keys_scratch(self.count))
        assert not self.kstat.any()
        self.host = buf.cpu().numpy()

    def requests(self):
        """[(stream, start, len)] in plaintext bytes, and the one served from the damaged chunk"""
        C = self.cls[PLAIN_NAMED]
        reqs = []
        for s, P in enumerate(PLAIN_SIZES):
            reqs += [(s, 0, min(P, 4096)), (s, max(P - 10, 0), 100)]
        reqs += [(PLAIN_NAMED, k * C - 97 - 20, 40) for k in (1, 2, 3)]
        reqs += [(PLAIN_NAMED, 5000 + 17 * sh, 33) for sh in range(16)]
        rebuilt = (PLAIN_NAMED, self.damaged[0] * C + self.damaged[1] * 1024 - 97 + 100, 300)
        return reqs + [rebuilt], len(reqs)

    def slices(self, reqs):
        return [np.frombuffer(self.pt[s][a:a + n], dtype=np.uint8) for s, a, n in reqs]


def test_plaintext_reads_and_the_key_table(gpu, far):
    """read_plain_ranges, read_plain_ranges_planned (also at a content stride
    past 4 GiB) and key_table_from_streams over far level-13 streams: the
    plaintexts, and the host-made key table."""
    import torch
    from types import SimpleNamespace
    from bao_damage import chunk_off
    from carbonado_amd import device as D
    import test_gpu_kread as TK
    src, dst = far
    w = PlainWorld()
    named = PLAIN_NAMED
    reqs, rebuilt = w.requests()
    nreq = len(reqs)
    rs, start, length = ([r[k] for r in reqs] for k in range(3))
    want = w.slices(reqs)
    want_vouch = [1 if r == rebuilt else 0 for r in range(nreq)]
    s_base = BASE(cut_for(w.off[named], w.len[named]))
    assert_straddles(s_base, w.off, w.len, named)
    src.put(w.host, s_base)
    far_off = _shifted(s_base, w.off)

    # host-planned, content far
    coff, clen, total, nseg = D.plain_read_layout(w.cls, w.pads, rs, start, length)
    assert clen == [p.size for p in want]
    big = reqs.index((named, 0, 4096))
    c_base = BASE(cut_for(coff[big], clen[big]))
    assert_straddles(c_base, coff, [max(n, 1) for n in clen], big)
    st, used, vouch = (torch.full((nreq,), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3))
    got = D.read_plain_ranges(w.keys, w.ivs, w.kstat, src.buf, far_off, w.len, w.hashes, w.pads, w.cls, rs, start, length,
                              dst.buf, _shifted(c_base, coff), st, used, vouch,
                              D.plain_read_scratch(nreq, nseg, w.count))
    torch.cuda.synchronize()
    assert got == clen and st.cpu().tolist() == [0] * nreq and vouch.cpu().tolist() == want_vouch
    assert bin(used.cpu().tolist()[rebuilt]).count("1") == 4 and not used.cpu().tolist()[rebuilt] & 2
    image = np.full(total, CANARY, dtype=np.uint8)
    for o, p in zip(coff, want):
        image[o:o + p.size] = p
    _same(dst.window(c_base, total, GUARD), _guarded(image), "read_plain_ranges")
    _only_written(dst, [(c_base, total)])
    _clean(dst, c_base, total)

    # device-planned over a stream table of the far offsets and the host-made key table
    table = D.stream_table(src.buf, far_off, w.len, w.hashes, w.pads, w.cls)
    host_made = D.key_table(w.keys, w.ivs, w.kstat)
    pw = SimpleNamespace(torch=torch, D=D, table=table, ktab=host_made)  # the world test_gpu_kread.Planned wants
    max_len = 4096
    stride = RW.up16(max_len) + 16
    p_base = BASE(cut_for(big * stride, max_len))
    assert_straddles(p_base, [r * stride for r in range(nreq)], [stride - 16] * nreq, big)
    runs = [(FarPlanned(TK.Planned(pw, nreq, max_len), dst, p_base, stride), reqs, want, want_vouch)]
    two = [reqs[big], reqs[rebuilt]]
    runs += [(FarPlanned(TK.Planned(pw, 2, max_len), dst, 0, FAR_PITCH), two, w.slices(two), [0, 1])]
    for fp, rq, exp, exp_vouch in runs:
        res = fp.run([(*r, 0) for r in rq])
        assert res.clen == [p.size for p in exp] and res.status.tolist() == [0] * len(rq)
        assert res.vouch.tolist() == exp_vouch
        for r, p in enumerate(exp):
            _same(res.content[r * stride:r * stride + p.size], p, ("planned request", rq[r]))
    _only_written(src, [(s_base, w.host.size)])
    _same(src.window(s_base, w.host.size), w.host, "a read changed the streams")
    _clean(dst, p_base, nreq * stride + 64)
    dst.refill([], low=stride + GUARD)
    _clean(src, s_base, w.host.size)

    # the key table from the streams: the first 81 envelope bytes of a small stream across 2^32
    small = PLAIN_SMALL
    head = w.off[small] + chunk_off(0, 8)  # chunk 0 of its eight: the envelope's first bytes
    k_base = BASE(head + 40)
    assert_straddles(k_base, w.off, w.len, small, side=16)
    assert FOUR_GIB - (k_base + head) >= 16 and k_base + head + 81 - FOUR_GIB >= 16
    src.put(w.host, k_base)
    table = D.stream_table(src.buf, _shifted(k_base, w.off), w.len, w.hashes, w.pads, w.cls)
    kt = D.key_table_from_streams(table, PLAIN_SECRET)
    torch.cuda.synchronize()
    assert kt.table.numel() == host_made.table.numel() and torch.equal(kt.table, host_made.table)
    _only_written(src, [(k_base, w.host.size)])
    _same(src.window(k_base, w.host.size), w.host, "the key table call changed the streams")
    for t in (kt, host_made):
        D.wipe_key_table(t)
    torch.cuda.synchronize()
    _clean(src, k_base, w.host.size)


# ---- snappy: the frame kernels and the one-call forms at 14 -----------------------------
SNAP_NAMES = ["random65537", "mix40_4097", "mix300_300", "mix40_65537", "zeros200000"]
SNAP_NAMED = 2   # mix300_300: raw and compressed chunks, two blocks


def _snap_objects():
    import snap_data as SD
    by = dict(SD.objects())
    return [by[name] for name in SNAP_NAMES]


def _image(size, offs, blobs, fill=CANARY):
    img = np.full(size, fill, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        img[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return img


def test_snap_and_unsnap_ragged(gpu, far):
    """snap_ragged and unsnap_ragged against the host stage's streams
    (chip_snap_compress, equal to the oracle's) and the content back."""
    import torch
    from carbonado_amd import device as D
    from oracle import oracle as O
    import snap_data as SD
    import test_gpu_snap_dev as TS
    src, dst = far
    datas, named = _snap_objects(), SNAP_NAMED
    lens = [len(d) for d in datas]
    frames = [TS.host_snap(d) for d in datas]
    assert frames == [O.c_snap_compress(d) for d in datas]
    assert {"raw", "compressed"} <= SD.kinds(frames[named]) and lens[named] == 2 * SD.BLOCK
    flen = [len(s) for s in frames]

    # compress: objects at 16-B aligned offsets, stream o at residue o % 16 with its worst-case room
    in_off, pos = [], 0
    for n in lens:
        in_off.append(pos)
        pos += RW.up16(n)
    in_size = pos + 16
    out_off, pos = [], 0
    for o, n in enumerate(lens):
        out_off.append(RW.up16(pos) + o % 16)
        pos = out_off[-1] + D.snap_max_len(n)
    out_size = pos + 64
    p_base = BASE(cut_for(in_off[named], lens[named]))
    f_base = BASE(cut_for(out_off[named], flen[named]))
    assert_straddles(p_base, in_off, lens, named)
    assert_straddles(f_base, out_off, flen, named)
    src.put(_image(in_size, in_off, datas, 0x11), p_base)
    out_len = torch.full((len(datas),), -1, dtype=torch.int64, device="cuda")
    D.snap_ragged(src.buf, _shifted(p_base, in_off), lens, dst.buf, _shifted(f_base, out_off), out_len,
                  D.snap_scratch(lens))
    torch.cuda.synchronize()
    assert out_len.cpu().tolist() == flen
    _same(dst.window(f_base, out_size, GUARD), _guarded(_image(out_size, out_off, frames)), "snap_ragged")
    _only_written(dst, [(f_base, out_size)])
    _only_written(src, [(p_base, in_size)])
    _clean(dst, f_base, out_size)
    _clean(src, p_base, in_size)

    # decompress: the streams at odd addresses, exact capacities
    s_off, pos = [], 1
    for s in frames:
        s_off.append(pos)
        pos += len(s) + (2 if len(s) % 2 == 0 else 1)
    s_size = pos + 16
    c_off, pos = [], 0
    for n in lens:
        c_off.append(pos)
        pos += RW.up16(n) + 16
    c_size = pos + 64
    s_base = BASE(cut_for(s_off[named], flen[named]))
    c_base = BASE(cut_for(c_off[named], lens[named]))
    assert_straddles(s_base, s_off, flen, named)
    assert_straddles(c_base, c_off, lens, named)
    src.put(_image(s_size, s_off, frames, 0x33), s_base)
    out_len = torch.full((len(datas),), -1, dtype=torch.int64, device="cuda")
    status = torch.full((len(datas),), 0x7777, dtype=torch.int32, device="cuda")
    D.unsnap_ragged(src.buf, _shifted(s_base, s_off), flen, dst.buf, _shifted(c_base, c_off), lens, out_len, status,
                    D.snap_scratch(flen, lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(datas) and out_len.cpu().tolist() == lens
    _same(dst.window(c_base, c_size, GUARD), _guarded(_image(c_size, c_off, datas)), "unsnap_ragged")
    _only_written(dst, [(c_base, c_size)])
    _only_written(src, [(s_base, s_size)])
    _clean(dst, c_base, c_size)
    _clean(src, s_base, s_size)


def test_snap_one_call_forms_at_14(gpu, far):
    """encode_ragged_snap and decode_ragged_snap at level 14 against the C oracle's encode."""
    import torch
    from carbonado_amd import device as D
    import test_gpu_snap_dev as TS
    src, dst = far
    named = SNAP_NAMED
    s = TS.Batch(14, _snap_objects(), seed=74)
    want = [s.oracle(o) for o in range(s.count)]
    s_len = [len(enc) for enc, _, _ in want]
    assert all(n <= c for n, c in zip(s_len, s.cap))
    size = s.total + 64
    streams = _image(size, s.out_off, [enc for enc, _, _ in want])
    p_base = BASE(cut_for(s.in_off[named], s.lens[named]))
    s_base = BASE(cut_for(s.out_off[named], s_len[named]))
    assert_straddles(p_base, s.in_off, s.lens, named)
    assert_straddles(s_base, s.out_off, s_len, named)

    src.put(s.plain_image(0x11), p_base)
    hashes = torch.full((s.count, 32), 0xEE, dtype=torch.uint8, device="cuda")
    olen, info = D.encode_ragged_snap(14, src.buf, _shifted(p_base, s.in_off), s.lens, dst.buf,
                                      _shifted(s_base, s.out_off), hashes, D.snap_ragged_scratch(14, s.lens))
    torch.cuda.synchronize()
    assert olen == s_len
    _same(dst.window(s_base, size, GUARD), _guarded(streams), "encode_ragged_snap")
    hh = hashes.cpu().numpy()
    for o, (_, h, winfo) in enumerate(want):
        assert bytes(hh[o]) == h, o
        TS._same_info(info[o], winfo)
    _only_written(dst, [(s_base, size)])
    _only_written(src, [(p_base, s.in_size)])
    _clean(dst, s_base, size)
    _clean(src, p_base, s.in_size)

    src.put(streams, s_base)
    hashes = RW.dev(np.frombuffer(b"".join(h for _, h, _ in want), dtype=np.uint8)).view(s.count, 32)
    pads = [winfo["padding_len"] for _, _, winfo in want]
    status = torch.full((s.count,), 0x7777, dtype=torch.int32, device="cuda")
    got = torch.full((s.count,), -1, dtype=torch.int64, device="cuda")
    D.decode_ragged_snap(14, src.buf, _shifted(s_base, s.out_off), s_len, hashes, pads, dst.buf,
                         _shifted(p_base, s.in_off), s.lens, got, status, D.snap_ragged_scratch(14, s_len, s.lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * s.count and got.cpu().tolist() == s.lens
    _same(dst.window(p_base, s.in_size, GUARD), _guarded(s.plain_image(CANARY)), "decode_ragged_snap")
    _only_written(dst, [(p_base, s.in_size)])
    _only_written(src, [(s_base, size)])
    _clean(dst, p_base, s.in_size)
    _clean(src, s_base, size)


# ---- slice audits planned on the device -------------------------------------------------
def _slots_hold(f: FW.Far, base, stride, blobs, what):
    """slot r of f at base + r * stride holds blobs[r], and nothing else of f was written"""
    if stride * len(blobs) <= ROOM:  # one window over all slots, the gaps between them included
        size = stride * len(blobs)
        _same(f.window(base, size, GUARD), _guarded(_image(size, [r * stride for r in range(len(blobs))], blobs)), what)
    else:
        for r, b in enumerate(blobs):
            _same(f.window(base + r * stride, len(b)), np.frombuffer(b, dtype=np.uint8), (what, r))
    _only_written(f, [(base + r * stride, len(b)) for r, b in enumerate(blobs)])
    f.refill([(base + r * stride, len(b)) for r, b in enumerate(blobs)])


def _put_slots(f: FW.Far, base, stride, blobs):
    for r, b in enumerate(blobs):
        if b:
            f.put(np.frombuffer(b, dtype=np.uint8), base + r * stride)


def test_planned_slice_audits(gpu, far):
    """verify_slices_planned, extract_slices_planned and
    verify_slice_proofs_planned over the audit streams: stream table of far
    offsets, proofs and content in far slots, then two requests at proof and
    content pitches of 2^32 + 256; against the Python oracle's slices, which
    test_gpu_paudit holds the host-planned calls to."""
    import torch
    from carbonado_amd import device as D
    from oracle import pyoracle as P
    import test_gpu_audit as TA
    from test_slice_verify import _grid
    src, dst = far
    made = [TA._stream(n) for n in AUDIT_SIZES]
    blobs, hash_list = [e for _, e, _ in made], [h for _, _, h in made]
    host, in_off = TA._pack_streams(blobs)
    in_len = [len(b) for b in blobs]
    k = len(blobs)
    N = -(-AUDIT_SIZES[AUDIT_NAMED] // 1024)
    reqs = [(s, i, c) for s, n in enumerate(AUDIT_SIZES) for i, c in _grid(n)]
    named = reqs.index((AUDIT_NAMED, 0, N))
    memo = [P.bao_prime(e, h) for e, h in zip(blobs, hash_list)]
    proofs = [P.bao_slice(blobs[s], i * 1024, c * 1024) for s, i, c in reqs]
    contents = [P.bao_decode_slice(proofs[r], hash_list[s], i * 1024, c * 1024, memo=memo[s])
                for r, (s, i, c) in enumerate(reqs)]
    hashes = RW.dev(np.frombuffer(b"".join(hash_list), dtype=np.uint8))
    s_base = BASE(cut_for(in_off[AUDIT_NAMED], in_len[AUDIT_NAMED]))
    assert_straddles(s_base, in_off, in_len, AUDIT_NAMED)
    src.put(host, s_base)
    table = D.stream_table(src.buf, _shifted(s_base, in_off), in_len, hashes, [0] * k, [1024] * k)
    roots = D.root_table(AUDIT_SIZES, hashes)
    assert (table.nstreams, table.max_chunks, roots.nroots, roots.max_chunks) == (k, N, k, N)
    cs = 1024 * N + 16
    ps = RW.up16(D.proof_bound(N, N)) + 16

    def tensors(rq):
        rs = torch.from_numpy(np.array([r[0] for r in rq], dtype=np.int32)).cuda()
        idx, cnt = (torch.tensor([r[j] for r in rq], dtype=torch.int64, device="cuda") for j in (1, 2))
        status = torch.full((len(rq) + 8,), -1, dtype=torch.int32, device="cuda")
        length = torch.full((len(rq) + 8,), -1, dtype=torch.int64, device="cuda")
        return rs, idx, cnt, status, length

    def served(status, length, blobs_):
        torch.cuda.synchronize()
        n = len(blobs_)
        assert status.cpu().tolist() == [0] * n + [-1] * 8
        assert length.cpu().tolist() == [len(b) for b in blobs_] + [-1] * 8

    two = [named, reqs.index((2, 1, 3))]
    # (requests, their proofs and contents, content base and stride, proof base and stride)
    runs = [(reqs, proofs, contents, BASE(cut_for(named * cs, len(contents[named]))), cs,
             BASE(cut_for(named * ps, len(proofs[named]))), ps),
            ([reqs[r] for r in two], [proofs[r] for r in two], [contents[r] for r in two], 0, FAR_PITCH, 0, FAR_PITCH)]
    nreq = len(reqs)
    assert_straddles(runs[0][3], [r * cs for r in range(nreq)], [cs - 16] * nreq, named)
    assert_straddles(runs[0][5], [r * ps for r in range(nreq)], [ps - 16] * nreq, named)
    assert len(contents[named]) == AUDIT_SIZES[AUDIT_NAMED] and len(proofs[named]) == in_len[AUDIT_NAMED]
    for rq, pr, co, c_base, c_stride, p_base, p_stride in runs:
        n = len(rq)
        scratch = D.planned_audit_scratch(table, n, N)
        rs, idx, cnt, status, clen = tensors(rq)
        D.verify_slices_planned(table, rs, idx, cnt, N, dst.buf[c_base:], c_stride, clen, status, scratch)
        served(status, clen, co)
        _slots_hold(dst, c_base, c_stride, co, "verify_slices_planned")

        rs, idx, cnt, status, plen = tensors(rq)
        D.extract_slices_planned(table, rs, idx, cnt, N, dst.buf[p_base:], p_stride, plen, status, scratch)
        served(status, plen, pr)
        _slots_hold(dst, p_base, p_stride, pr, "extract_slices_planned")
    _only_written(src, [(s_base, host.size)])
    _same(src.window(s_base, host.size), host, "an audit changed the streams")
    _clean(src, s_base, host.size)

    # the auditor's side: the oracle's proofs in far slots of src, content into far slots of dst
    for rq, pr, co, c_base, c_stride, p_base, p_stride in runs:
        n = len(rq)
        _put_slots(src, p_base, p_stride, pr)
        rs, idx, cnt, status, clen = tensors(rq)
        plen = torch.tensor([len(p) for p in pr], dtype=torch.int64, device="cuda")
        D.verify_slice_proofs_planned(roots, rs, idx, cnt, N, src.buf[p_base:], p_stride, plen, dst.buf[c_base:],
                                      c_stride, clen, status, D.planned_audit_scratch(roots, n, N))
        served(status, clen, co)
        _slots_hold(dst, c_base, c_stride, co, "verify_slice_proofs_planned")
        _slots_hold(src, p_base, p_stride, pr, "verify_slice_proofs_planned changed the proofs")
    for f in far:
        f.refill([], low=nreq * max(cs, ps) + GUARD)


# ---- plaintext reads of level-14 streams: the frame index, the reads --------------------
FRAME_NAMED = 6   # 131077 bytes: three frames; the four-frame stream behind it lies entirely above


class _FramePlanned(RW.Planned):
    """read_frame_ranges_planned at 14 over the world w: torch, D, table (stream table), frames (frame table)"""

    def scratch_len(self):
        return self.w.D.planned_frame_read_scratch(self.table, self.w.frames, self.nreq, self.max_len).numel()

    def enqueue(self, flags=0):
        self.w.D.read_frame_ranges_planned(self.table, self.w.frames, None, self.rs, self.start, self.length,
                                           self.max_len, self.content, self.stride, self.clen, self.status, self.used,
                                           self.vouch, self.scratch, flags)


def test_frame_index_and_frame_reads(gpu, far):
    """frame_index, read_frame_ranges and read_frame_ranges_planned (also at a
    content stride past 4 GiB) over the level-14 streams of test_gpu_fread moved
    across 2^32: the Python walk of the host's frame streams, the plaintexts,
    and the host-planned call as test_gpu_gread compares it."""
    import torch
    from types import SimpleNamespace
    from carbonado_amd import device as D
    import test_gpu_fread as TF
    import test_gpu_gread as TG
    src, dst = far
    fmt, named = 14, FRAME_NAMED
    s = TF.streams(fmt)
    assert s.nframes[named] >= 3
    size = s.out.numel()
    host = s.out.cpu().numpy()
    s_base = BASE(cut_for(s.off[named], s.olen[named]))
    assert_straddles(s_base, s.off, s.olen, named)
    src.put(s.out, s_base)
    far_off = _shifted(s_base, s.off)

    caps = [n + 1 for n in s.nframes]
    frame_off, nframes, status, plain, vouch = D.frame_index(fmt, src.buf, far_off, s.olen, s.hashes, s.pads, s.cls,
                                                             s.idx_off, caps, D.frame_index_scratch(s.count, sum(caps)))
    assert status.tolist() == [0] * s.count and vouch.tolist() == [0] * s.count
    assert nframes.tolist() == s.nframes and plain.tolist() == TF.SIZES
    for o, i in zip(s.idx_off, s.index):
        assert frame_off[o:o + len(i)].tolist() == i

    # host-planned, content far at every residue mod 16
    reqs = TF.requests()
    rs, start, length = ([r[k] for r in reqs] for k in range(3))
    want = [np.frombuffer(s.pt[o][a:a + n], dtype=np.uint8) for o, a, n in reqs]
    _, clen, _, nseg, stage, vseg = D.frame_read_layout(fmt, s.cls, s.pads, s.frame_off, s.idx_off, s.nframes, TF.SIZES,
                                                        rs, start, length)
    assert clen == [p.size for p in want]
    coff, at = [], 5
    for r, n in enumerate(clen):
        at += (r * 7) % 16 + 1
        coff.append(at)
        at += n
    total = at + 40
    big = reqs.index((named, 0, TF.SIZES[named]))
    c_base = BASE(cut_for(coff[big], clen[big]))
    assert_straddles(c_base, coff, [max(n, 1) for n in clen], big)
    st, used, vo = (torch.full((len(reqs),), 0x7777, dtype=torch.int32, device="cuda") for _ in range(3))
    got = D.read_frame_ranges(fmt, src.buf, far_off, s.olen, s.hashes, s.pads, s.cls, s.frame_off, s.idx_off, s.nframes,
                              TF.SIZES, rs, start, length, dst.buf, _shifted(c_base, coff), st, used, vo,
                              D.frame_read_scratch(len(reqs), nseg, stage, vseg, s.count))
    torch.cuda.synchronize()
    assert got == clen and st.cpu().tolist() == [0] * len(reqs) and vo.cpu().tolist() == [0] * len(reqs)
    _same(dst.window(c_base, total, GUARD), _guarded(_image(total, coff, [p.tobytes() for p in want])), "read_frame_ranges")
    _only_written(dst, [(c_base, total)])
    _clean(dst, c_base, total)

    # device-planned: stream table of the far offsets, content slots far
    pw = SimpleNamespace(torch=torch, D=D,
                         table=D.stream_table(src.buf, far_off, s.olen, s.hashes, s.pads, s.cls),
                         frames=D.frame_table(fmt, s.cls, s.pads, s.frame_off, s.idx_off, s.nframes, TF.SIZES))
    low = TG.world(fmt)
    max_len = 4096
    stride = RW.up16(max_len) + 16
    preqs = TG.base_requests(max_len)
    big = preqs.index((named, 0, max_len, 0))
    p_base = BASE(cut_for(big * stride, max_len))
    assert_straddles(p_base, [r * stride for r in range(len(preqs))], [stride - 16] * len(preqs), big)
    res = FarPlanned(_FramePlanned(pw, len(preqs), max_len), dst, p_base, stride).run(preqs)
    assert res.clen[big] == max_len
    RW.assert_equal(res, TG.reference(low, preqs, stride), preqs)
    two = [(named, TF.FRAME - 100, max_len, 0), (TF.BIG, 2 * TF.FRAME + 17, 300, 0)]
    res = FarPlanned(_FramePlanned(pw, 2, max_len), dst, 0, FAR_PITCH).run(two)
    for r, (o, a, n, _) in enumerate(two):  # both slots hold the plaintexts
        _same(res.content[r * stride:r * stride + n], np.frombuffer(s.pt[o][a:a + n], dtype=np.uint8), ("slot", r))
    RW.assert_equal(res, TG.reference(low, two, stride), two)
    _only_written(src, [(s_base, size)])
    _same(src.window(s_base, size), host, "a read changed the streams")
    _clean(dst, p_base, len(preqs) * stride + 64)
    dst.refill([], low=stride + GUARD)
    _clean(src, s_base, size)
