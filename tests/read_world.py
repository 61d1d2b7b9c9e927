"""What the GPU tests of the read families share: small buffer helpers, the
streams of the plaintext-read tests (cread, fread), and the comparison of a
device-planned read with the host-planned call over the same requests (qread,
kread).  Every fill, canary and guard value of those tests is stated here."""
import numpy as np

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)

CANARY, GUARD = 0xC7, 0x5B


def up16(x: int) -> int:
    return (x + 15) // 16 * 16


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


# ---- the resident streams of the plaintext-read tests ---------------------------------
class PlainStreams:
    """The base of a test's Streams: self.pt (the plaintexts, bytes) comes
    first; the encode call gives self.off and self.cls (stream offsets, shard
    lengths); the encode call, the index and the calls under test are the
    subclass's."""

    def place_plain(self, sizes):
        """(in_off, image): the plaintexts at pitches of up16(n) + 16 in a 0x11 fill."""
        in_off, at = [], 0
        for n in sizes:
            in_off.append(at)
            at += up16(n) + 16
        plain = np.full(at + 16, 0x11, dtype=np.uint8)
        for o, n in enumerate(sizes):
            plain[in_off[o]:in_off[o] + n] = np.frombuffer(self.pt[o], dtype=np.uint8)
        return in_off, plain

    def make_outputs(self, total, count):
        """self.out (0xA5, 64 bytes more than the layout's total) and self.hashes (0xEE) for the encode call"""
        import torch
        self.out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.hashes = torch.full((count, 32), 0xEE, dtype=torch.uint8, device="cuda")

    def chunk_pos(self, s, chunk, byte):
        """Where byte `byte` of chunk `chunk` of stream s lies in self.out."""
        return self.off[s] + B.chunk_offsets(self.cls[s] // 1024)[chunk] + byte

    def flipped(self, positions):
        """A copy of the streams with one bit (0x40) flipped at each position."""
        out = self.out.clone()
        for at in positions:
            out[at] ^= 0x40
        return out

    def want(self, reqs, coff, size, zero=(), pt=None):
        """The content image: slices of the plaintexts (zeros for the requests in `zero`) in a 0xA5 fill."""
        img = np.full(size, 0xA5, dtype=np.uint8)
        for r, (s, a, n) in enumerate(reqs):
            part = np.frombuffer((pt or self.pt)[s][a:a + n], dtype=np.uint8)
            img[coff[r]:coff[r] + part.size] = 0 if r in zero else part
        return img


# ---- device-planned reads against the host-planned call --------------------------------
class Got:
    def __init__(self, status, used, vouch, clen, content):
        self.status, self.used, self.vouch, self.clen, self.content = status, used, vouch, clen, content


def _check_canary(content, clen, stride):
    rows = content[:len(clen) * stride].reshape(len(clen), stride)
    outside = np.arange(stride)[None, :] >= np.asarray(clen)[:, None]
    assert (rows[outside] == CANARY).all(), "a byte outside [0, content_len) of a slot was written"
    assert (content[len(clen) * stride:] == CANARY).all()


class Planned:
    """Device buffers of one capacity (nreq, max_len) over the world w (w.torch,
    w.D, w.table); run() as often as wanted.  A subclass gives scratch_len()
    and enqueue(flags), and sets vouched = False where its call fills no vouch
    words."""
    vouched = True

    def __init__(self, w, nreq, max_len, table=None):
        torch = w.torch
        self.w, self.nreq, self.max_len = w, nreq, max_len
        self.table = table or w.table
        self.stride = (max_len + 15) // 16 * 16 + 16
        self.rs = torch.zeros(nreq, dtype=torch.int32, device="cuda")
        self.start = torch.zeros(nreq, dtype=torch.int64, device="cuda")
        self.length = torch.zeros(nreq, dtype=torch.int64, device="cuda")
        need = self.scratch_len()
        self.full = torch.full((need + 256,), GUARD, dtype=torch.uint8, device="cuda")
        self.scratch = self.full[:need]
        self.content = torch.full((nreq * self.stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
        self.clen = torch.full((nreq,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((nreq + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.used = torch.full((nreq + 8,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
        self.vouch = torch.full((nreq + 8,), 0x69696969, dtype=torch.int32, device="cuda")

    def scratch_len(self) -> int:
        raise NotImplementedError

    def enqueue(self, flags=0):
        raise NotImplementedError

    def set(self, reqs):
        torch = self.w.torch
        self.rs.copy_(torch.tensor([r[0] for r in reqs], dtype=torch.int32))
        self.start.copy_(torch.tensor([r[1] for r in reqs], dtype=torch.int64))
        self.length.copy_(torch.tensor([r[2] for r in reqs], dtype=torch.int64))
        self.content.fill_(CANARY)

    def result(self) -> Got:
        torch, n = self.w.torch, self.nreq
        torch.cuda.synchronize()
        assert (self.full[self.scratch.numel():] == GUARD).all().item(), "bytes behind scratch_len were written"
        assert (self.status[n:] == 0x5A5A5A5A).all().item() and (self.used[n:] == 0x3C3C3C3C).all().item()
        assert (self.vouch[n if self.vouched else 0:] == 0x69696969).all().item()
        got = Got(self.status[:n].cpu().numpy(), self.used[:n].cpu().numpy(),
                  self.vouch[:n].cpu().numpy() if self.vouched else None, self.clen.cpu().numpy().tolist(),
                  self.content.cpu().numpy())
        _check_canary(got.content, got.clen, self.stride)
        return got

    def run(self, reqs, flags=0) -> Got:
        self.set(reqs)
        self.enqueue(flags)
        return self.result()


def host_requests(reqs, stride):
    """(req_stream, start, length, content_off) of the host-planned reference
    over reqs = [(stream, start, len, refused)]: request r at r * stride, a
    refused request as an empty range of stream 0."""
    rs = [0 if r[3] else r[0] for r in reqs]
    start = [0 if r[3] else r[1] for r in reqs]
    length = [0 if r[3] else r[2] for r in reqs]
    return rs, start, length, [r * stride for r in range(len(reqs))]


def host_result(reqs, clen, content, status, used, vouch=None) -> Got:
    """The reference as the planned call words it: what the host-planned call
    gave (device tensors, synchronised here), with status 1, used 0 and vouch 0
    for a refused request, whose empty range must have read nothing."""
    import torch
    torch.cuda.synchronize()
    status, used = status.cpu().numpy(), used.cpu().numpy()
    vouch = vouch.cpu().numpy() if vouch is not None else None
    for r, rq in enumerate(reqs):
        if rq[3]:
            assert clen[r] == 0
            status[r], used[r] = 1, 0
            if vouch is not None:
                vouch[r] = 0
    return Got(status, used, vouch, clen, content.cpu().numpy())


def assert_equal(got: Got, want: Got, reqs):
    assert got.clen == want.clen, [(r, reqs[r], a, b) for r, (a, b) in enumerate(zip(got.clen, want.clen)) if a != b][:8]
    for name in ("status", "used", "vouch"):
        a, b = getattr(got, name), getattr(want, name)
        if b is None:
            continue
        bad = [(name, r, reqs[r], int(a[r]), int(b[r])) for r in np.flatnonzero(a != b)[:8]]
        assert not bad, bad
    if not np.array_equal(got.content, want.content):
        at = int(np.flatnonzero(got.content != want.content)[0])
        raise AssertionError(f"content differs at byte {at}")
