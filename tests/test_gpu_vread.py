"""read_ranges_vouched (include/carbonado_hip_vread.h) against the independent
oracle.  The class of every segment comes from oracle/pyoracle.py and the C
oracle, never from the code under test:

  * whether slice (segment, shard) is authentic: `_verdict` of
    test_gpu_read_ranges.py (bao_decode_slice over bao_slice of the damaged
    stream);
  * PATH(g): bao_decode_slice accepts the primary's slice of the damaged stream
    with the window's chunks put back from the clean stream;
  * VOUCHED against CONTRADICTED: the C oracle's zfec decode of the four
    selected shares' window chunks, compared with the clean stream's chunks of
    the primary.

Status, used, vouch and content follow from the classes by the header's rule
and are exact.  "Clean" is the stream as it was bao-encoded; for the
contradiction cases that is a stream over eight shards that are no valid zfec
encoding, which every hash in it vouches for all the same."""
import functools
import random
from typing import NamedTuple

import numpy as np
import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
import test_gpu_read_ranges as RR
from oracle import oracle as O
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SENT, GUARD = RR.SENT, RR.GUARD
VOUCHED, UNVOUCHED, CONTRADICTED, STRICT = 1, 2, 4, 1
DIRECT, FAILED = "direct", "failed"


class VWant(NamedTuple):
    status: int      # with flags = 0
    strict: int      # with CHIPV_STRICT
    used: int        # where the status is 0
    vouch: int
    content: bytes   # where the status is 0
    classes: tuple


def _window(stream: bytes, spc: int, shard: int, w0: int, w1: int) -> bytes:
    off = B.chunk_offsets(spc)
    return b"".join(stream[off[shard * spc + c]:off[shard * spc + c] + 1024] for c in range(w0, w1))


def _path_holds(st, bad: bytes, p: int, w0: int, w1: int) -> bool:
    fixed = bytearray(bad)
    off = B.chunk_offsets(st.spc)
    for c in range(p * st.spc + w0, p * st.spc + w1):
        fixed[off[c]:off[c] + 1024] = st.clean[off[c]:off[c] + 1024]
    start, ln = (p * st.spc + w0) * 1024, (w1 - w0) * 1024
    try:
        P.bao_decode_slice(P.bao_slice(bytes(fixed), start, ln), st.hash, start, ln, st.memo)
        return True
    except P.SliceError:
        return False


def vexpected(streams, reqs):
    """VWant per request."""
    bads = [st.bad for st in streams]
    caches = [{} for _ in streams]
    seg_class = {}
    out = []
    for rq in reqs:
        st, bad = streams[rq.stream], bads[rq.stream]
        segs = RR._segments(st, rq.start, rq.len)
        size = sum(c1 - c0 for _, c0, c1 in segs)
        used, vouch, failed, classes = 0, 0, False, []
        for p, c0, c1 in segs:
            w0, w1 = c0 // 1024, -(-c1 // 1024)
            key = (rq.stream, p, w0, w1)
            if key not in seg_class:
                v = functools.partial(RR._verdict, st, bad, caches[rq.stream], w0=w0, w1=w1)
                if v(p):
                    seg_class[key] = (DIRECT, 1 << p)
                else:
                    good = [i for i in range(8) if i != p and v(i)]
                    if len(good) < 4:
                        seg_class[key] = (FAILED, 0)
                    else:
                        sel = good[:4]
                        bits = sum(1 << i for i in sel)
                        if not _path_holds(st, bad, p, w0, w1):
                            seg_class[key] = (UNVOUCHED, bits)
                        else:
                            dec = O.zfec_decode_shares([_window(bad, st.spc, i, w0, w1) for i in sel], sel, 0)
                            L = 1024 * (w1 - w0)
                            same = dec[p * L:(p + 1) * L] == _window(st.clean, st.spc, p, w0, w1)
                            seg_class[key] = (VOUCHED if same else CONTRADICTED, bits)
            cls, bits = seg_class[key]
            classes.append(cls)
            used |= bits
            failed |= cls == FAILED
            vouch |= cls if isinstance(cls, int) else 0
        status = 5 if vouch & CONTRADICTED else 7 if failed else 0
        strict = 5 if vouch & CONTRADICTED else 7 if failed or vouch & UNVOUCHED else 0
        out.append(VWant(status, strict, used, vouch, st.data[rq.start:rq.start + size], tuple(classes)))
    return out


def _want(vw, strict=False):
    """RR.Want of every request for RR._check."""
    return [RR.Want(s, 0 if s else w.used, bytes(len(w.content)) if s else w.content)
            for w in vw for s in [w.strict if strict else w.status]]


class VCall(RR.Call):
    """RR.Call's buffers plus the vouch words and a scratch of the vouched call's length."""

    def __init__(self, streams, reqs, **kw):
        super().__init__(streams, reqs, **kw)
        torch, n = self.torch, len(reqs)
        need = self.D.vread_scratch(n, self.nseg).numel()
        assert need >= self.scratch.numel() and need % 16 == 0
        self.vfull = torch.full((need + 256,), GUARD, dtype=torch.uint8, device="cuda")
        self.vscratch = self.vfull[:need]
        self.vouch = torch.full((n + 8,), 0x69696969, dtype=torch.int32, device="cuda")

    def vread(self, flags=0):
        torch, n = self.torch, len(self.reqs)
        clen = self.D.read_ranges_vouched(self.inp, self.in_off, self.in_len, self.hashes, self.pads, self.cls, self.rs,
                                          self.start, self.len, self.content, self.off, self.status, self.used, self.vouch,
                                          self.vscratch, flags)
        torch.cuda.synchronize()
        assert (self.vfull[self.vscratch.numel():] == GUARD).all().item(), "bytes past scratch_len were written"
        assert np.array_equal(self.inp.cpu().numpy(), self.host), "read_ranges_vouched changed its input"
        assert (self.status[n:] == 0x5A5A5A5A).all().item() and (self.used[n:] == 0x3C3C3C3C).all().item()
        assert (self.vouch[n:] == 0x69696969).all().item()
        res = RR.Result(self.status[:n].cpu().numpy(), self.used[:n].cpu().numpy(), self.content.cpu().numpy(), self.off,
                        clen)
        return res, self.vouch[:n].cpu().numpy()


def _check(call, got, vw, strict=False):
    res, vouch = got
    RR._check(call, res, _want(vw, strict))
    bad = [(r, int(vouch[r]), w.vouch, w.classes) for r, w in enumerate(vw) if vouch[r] != w.vouch]
    assert not bad, bad[:8]


@functools.lru_cache(maxsize=None)
def main_vexpected():
    return tuple(vexpected(*RR.main_set()))


@functools.lru_cache(maxsize=None)
def main_vcall() -> VCall:
    return VCall(*RR.main_set())


@functools.lru_cache(maxsize=None)
def main_vresult():
    return main_vcall().vread()


def test_parity_every_size_range_and_damage_in_one_call(gpu):
    streams, reqs = RR.main_set()
    vw, want = main_vexpected(), RR.main_expected()
    assert len(streams) == 305 and len(reqs) == 2874
    # every stream here is a valid encoding: nothing is contradicted, and the old call's expectation holds
    assert _want(vw) == list(want) and not any(w.vouch & CONTRADICTED for w in vw)
    # nothing vacuous: vouched, unvouched and failed requests are all there, where the damage was built for them
    by = {(st.spc, st.what): s for s, st in enumerate(streams)}
    pick = {(st, a): vw[r] for r, (st, a, _) in enumerate(reqs)}
    for spc in RR.SPCS:
        focus = 1024 * spc + 1024 * RR._focus(spc) + 133
        assert pick[by[spc, "none"], focus].vouch == 0 and pick[by[spc, "none"], focus].classes == (DIRECT,)
        assert pick[by[spc, "chunk"], focus].vouch == VOUCHED and pick[by[spc, "chunk"], focus].status == 0
        assert pick[by[spc, "level-1 parent"], focus].vouch == UNVOUCHED
        assert pick[by[spc, "level-1 parent"], focus].status == 0 and pick[by[spc, "level-1 parent"], focus].strict == 7
        assert pick[by[spc, "four shards"], focus].vouch == VOUCHED
        assert pick[by[spc, "five shards"], focus].status == 7 and pick[by[spc, "five shards"], focus].vouch == 0
    assert sum(w.vouch == VOUCHED for w in vw) > 500 and sum(w.vouch == UNVOUCHED for w in vw) >= 7
    assert sum(w.status == 7 for w in vw) > 100
    _check(main_vcall(), main_vresult(), vw)


def test_agreement_with_read_ranges(gpu):
    call = main_vcall()
    (mine, _) = main_vresult()
    theirs = call.read()  # device.read_ranges over the same buffers
    assert np.array_equal(mine.status, theirs.status) and np.array_equal(mine.used, theirs.used)
    assert np.array_equal(mine.content, theirs.content) and mine.clen == theirs.clen


def test_strict_fails_exactly_the_unvouched(gpu):
    vw = main_vexpected()
    call, (base, _) = main_vcall(), main_vresult()
    got = call.vread(STRICT)
    _check(call, got, vw, strict=True)
    res, vouch = got
    turned = [r for r, w in enumerate(vw) if w.vouch & UNVOUCHED and w.status == 0]
    assert len(turned) >= 7
    for r, w in enumerate(vw):
        if r in turned:
            assert res.status[r] == 7 and res.used[r] == 0
            assert not res.content[res.off[r]:res.off[r] + res.clen[r]].any()
        else:
            assert res.status[r] == base.status[r] and res.used[r] == base.used[r]
            assert np.array_equal(res.content[res.off[r]:res.off[r] + res.clen[r]],
                                  base.content[res.off[r]:res.off[r] + res.clen[r]])


def test_repeat_over_dirty_buffers(gpu):
    """The same call again over its own leftovers: the scratch holds the last
    call's words, status, used and vouch are garbage, the content ranges hold
    another pattern: every word and byte is set again."""
    call, (first, fvouch) = main_vcall(), main_vresult()
    call.vread(0)  # (the strict test may have run last)
    n = len(call.reqs)
    call.status[:n] = 0x7F7F7F7F
    call.used[:n] = -1
    call.vouch[:n] = -1
    call.vscratch[call.vscratch.numel() // 2:] = 0xFF  # the words behind the uploaded table
    for r, w in enumerate(main_vexpected()):
        if w.content:
            call.content[call.off[r]:call.off[r] + len(w.content)] = 0xEE
    again = call.vread(0)
    _check(call, again, main_vexpected())
    assert np.array_equal(again[0].status, first.status) and np.array_equal(again[0].used, first.used)
    assert np.array_equal(again[1], fvouch)


# ---- streams over shards that are altered before they are hashed ------------------

def _built(spc: int, seed, what: str, alter=(), damage=lambda nodes, chunks, rng: []) -> RR.Stream:
    """The object's eight zfec shards with the bytes of `alter` ((shard, column,
    xor mask)) changed, bao-encoded as they then stand by the C oracle, whose
    decoder accepts the stream under its new hash; then `damage` as in
    test_gpu_read_ranges._stream.  `data` = the primaries as hashed."""
    d = random.Random(repr(seed)).randbytes(4096 * spc - 37 - spc)
    z, pad, C = O.zfec_encode(d)
    assert (pad, C) == (37 + spc, 1024 * spc)
    shards = bytearray(z)
    for shard, col, mask in alter:
        shards[shard * C + col] ^= mask
    enc, h = O.bao_encode(bytes(shards))
    assert O.bao_decode(enc, h) == bytes(shards)  # it verifies as bao, valid zfec or not
    if not alter:
        assert (enc, h) == O.encode(d, 12)[:2]
    nodes = B.tree_nodes(8192 * spc)
    chunks = [k for k, nd in enumerate(nodes) if not nd.parent]
    rng = random.Random(f"vread{seed}")
    flips = tuple(x[1:] if x[0] == "raw" else B.pick(nodes, x, rng) for x in damage(nodes, chunks, rng))
    return RR.Stream(spc, bytes(shards[:4 * C - pad]), enc, flips, h, pad, C, what, P.bao_prime(enc, h, {})), d


CONTRA_SPCS = [1, 2, 3, 9, 33]
COL = 517  # the altered column of the focus chunk


@functools.lru_cache(maxsize=None)
def contra_set(variant: int):
    """variant 0: the wrong share is secondary 4; variant 1: primary 1.  Primary
    0's focus chunk is damaged, so its ranges there are rebuilt from 1, 2, 3, 4."""
    streams, objs, reqs = [], [], []
    for spc in CONTRA_SPCS:
        j, C = RR._focus(spc), 1024 * spc
        wrong = 4 if variant == 0 else 1
        st, d = _built(spc, ("contra", variant, spc), f"shard {wrong} altered", alter=[(wrong, 1024 * j + COL, 0x40)],
                       damage=lambda nodes, chunks, rng, j=j: [(chunks[j], -1)])
        # before the damage all eight slices of the focus window are authentic
        whole = RR.Stream(*st[:3], (), *st[4:])
        assert all(RR._verdict(whole, st.clean, {}, i, j, j + 1) for i in range(8))
        s = len(streams)
        reqs += [RR.Req(s, 1024 * j + 100, 50), RR.Req(s, 1024 * j + 500, 40), RR.Req(s, 2 * C + 1024 * j + 11, 300)]
        if spc >= 2:
            reqs.append(RR.Req(s, 1024 * ((j + 1) % spc) + 7, 100))
        streams.append(st)
        objs.append(d)
    return tuple(streams), tuple(objs), tuple(reqs)


@pytest.mark.parametrize("variant", [0, 1])
def test_contradiction(gpu, variant):
    streams, objs, reqs = contra_set(variant)
    vw = vexpected(streams, reqs)
    r = 0
    for spc in CONTRA_SPCS:
        k = 4 if spc >= 2 else 3
        assert [(w.status, w.strict, w.vouch, w.classes) for w in vw[r:r + 2]] == [(5, 5, 4, (CONTRADICTED,))] * 2
        assert all((w.status, w.vouch, w.classes) == (0, 0, (DIRECT,)) for w in vw[r + 2:r + k])
        assert vw[r + 2].used == 0b100 and all(w.used == 0b1 for w in vw[r + 3:r + k])
        r += k
    assert r == len(reqs)
    call = VCall(streams, reqs)
    got = call.vread(0)
    _check(call, got, vw)
    res, vouch = got
    for r, w in enumerate(vw):
        if w.status == 5:
            assert res.used[r] == 0 and vouch[r] == 4 and not res.content[res.off[r]:res.off[r] + res.clen[r]].any()
    _check(call, call.vread(STRICT), vw, strict=True)
    # the gap this call closes: read_ranges serves the same requests with status 0, and wrong bytes where the
    # range holds the altered column
    old = call.read()
    for r, (rq, w) in enumerate(zip(reqs, vw)):
        assert old.status[r] == 0
        served = old.content[old.off[r]:old.off[r] + old.clen[r]].tobytes()
        obj = objs[rq.stream][rq.start:rq.start + rq.len]
        if w.status == 5:
            assert old.used[r] == 0b11110
            inside = rq.start % 1024 <= COL < rq.start % 1024 + rq.len
            assert (served != obj) == inside, r
            if inside:
                assert [i for i in range(rq.len) if served[i] != obj[i]] == [COL - rq.start % 1024]
        else:
            assert served == obj


# ---- one request, four segments, several classes -----------------------------------

def _mixed(variant: str):
    """spc 3, one request from chunk 1 of primary 0 to chunk 1 of primary 3:
    windows [1, 3), all, all, [0, 2)."""
    spc, C = 3, 3072

    def damage(nodes, chunks, rng):
        (par,) = [k for k, nd in enumerate(nodes) if nd.level == 1 and nd.lo <= 2 * spc < nd.hi]  # over chunks 6, 7
        out = [(chunks[spc + 1], -1), (par, rng.randrange(2))]
        if variant != "served":
            out += [(chunks[2], -1)] + [(chunks[i * spc], -1) for i in (3, 4, 5, 6, 7)]
        return out
    alter = [(3, 2048 + 99, 0x01)] if variant == "contradicted and failed" else []
    st, _ = _built(spc, ("mixed", variant), variant, alter=alter, damage=damage)
    return (st,), (RR.Req(0, 1024 + 10, 3 * C + 1024 + 100 - (1024 + 10)), RR.Req(0, 2 * C + 2048 + 5, 20))


@pytest.mark.parametrize("variant,classes,status,strict,vouch", [
    ("served", (DIRECT, VOUCHED, UNVOUCHED, DIRECT), 0, 7, 3),
    ("vouched and failed", (VOUCHED, FAILED, FAILED, FAILED), 7, 7, 1),
    ("contradicted and failed", (CONTRADICTED, FAILED, FAILED, FAILED), 5, 5, 4),
])
def test_four_segments_in_different_classes(gpu, variant, classes, status, strict, vouch):
    streams, reqs = _mixed(variant)
    vw = vexpected(streams, reqs)
    assert (vw[0].classes, vw[0].status, vw[0].strict, vw[0].vouch) == (classes, status, strict, vouch)
    if variant == "served":
        assert vw[0].used == 0b111001 and (vw[1].status, vw[1].vouch, vw[1].classes) == (0, 0, (DIRECT,))
    call = VCall(streams, reqs)
    _check(call, call.vread(0), vw)
    _check(call, call.vread(STRICT), vw, strict=True)


def test_one_16_mib_object(gpu):
    """N = 32768 chunks: a 4 KiB read across a damaged chunk deep inside primary
    1 is rebuilt from shards 0, 2, 3, 4 and vouched for; its neighbour is direct."""
    spc = 4096
    d = np.random.default_rng(16).integers(0, 256, (16 << 20) - 41, dtype=np.uint8).tobytes()
    enc, h, info = O.encode(d, 12)
    assert info["chunk_len"] == 1024 * spc and info["padding_len"] == 41
    nodes = B.tree_nodes(8192 * spc)
    k = next(j for j, nd in enumerate(nodes) if not nd.parent and nd.lo == spc + 1234)
    flips = (B.pick(nodes, (k, -1), random.Random(16)),)
    st = RR.Stream(spc, d, enc, flips, h, 41, 1024 * spc, "chunk 1234 of shard 1", P.bao_prime(enc, h, {}))
    C = 1024 * spc
    reqs = (RR.Req(0, C + 1024 * 1234 - 1500, 4096), RR.Req(0, C + 1024 * 1236 + 3, 4096))
    vw = vexpected((st,), reqs)
    assert [(w.status, w.used, w.vouch) for w in vw] == [(0, 0b11101, VOUCHED), (0, 0b10, 0)]
    assert vw[0].content == d[reqs[0].start:reqs[0].start + 4096]
    call = VCall((st,), reqs)
    _check(call, call.vread(STRICT), vw, strict=True)
