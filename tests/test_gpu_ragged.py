"""Ragged device batches (include/carbonado_hip_ext.h, carbonado_amd.device
encode_ragged / decode_ragged): objects of different lengths in one call,
every object's bytes, length, EncodeInfo, hash and status against the CPU
oracle (oracle.oracle = the reference's encode()/decode()).

SIZES are the smallest lengths at which the per-object tree can go wrong.  At
level 12 they give N = 8 and 16 (root inside the group), 64 (exactly one
group), 72 (a full group + a group of 8), 128, 136, 392 (7 groups: an odd
promotion in the top walk), 512, 520, 2048 and 2056 chunks; at level 4 N = 1
with 0 / 1 / 63 / 64 / 65 bytes, N = 2 with a 1-byte second chunk, N = 3 (odd
promotion), N = 64 and 65 with a second group of one chunk of 1 byte or full.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from bao_damage import chunk_off  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072, 4095, 4096, 4097, 8192,
         32768, 32769, 65535, 65536, 65537, 66560, 131073, 200001, 262144, 266240,
         1 << 20, (1 << 20) + 5]
LEVELS = [4, 8, 12]
GUARD = 4096
INFO_FIELDS = ("input_len", "output_len", "bytes_compressed", "compression_factor", "bytes_encrypted", "bytes_ecc",
               "bytes_verifiable", "amplification_factor", "padding_len", "chunk_len", "verifiable_slice_count",
               "chunk_slice_count")


@functools.lru_cache(maxsize=None)
def _data(n: int) -> bytes:
    return np.random.default_rng(7000 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _oracle(n: int, level: int):
    """(encoding, hash, info) of the reference's encode() of _data(n); computed once."""
    return O.encode(_data(n), level)


def _same_float(a: float, b: float) -> bool:  # f32 on both sides; 0 / 0 at an empty input is NaN on both
    a, b = np.float32(a), np.float32(b)
    return bool(a == b) or (math.isnan(a) and math.isnan(b))


def _check_info(got, want: dict, ctx):
    for f in INFO_FIELDS:
        g, w = getattr(got, f), want[f]
        assert _same_float(g, w) if isinstance(w, float) else g == w, (ctx, f, g, w)


def _pack(blobs, align=16, gap=16, fill=0x5A):
    """blobs at `align`-aligned offsets of one host buffer with `fill` gaps."""
    offs, cur = [], gap
    for b in blobs:
        offs.append(cur)
        cur += (len(b) + align - 1) // align * align + gap
    host = np.full(cur, fill, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return host, offs


def _untouched(buf: np.ndarray, offs, lens, fill=0xA5) -> bool:
    mask = np.ones(buf.size, dtype=bool)
    for o, n in zip(offs, lens):
        mask[o:o + n] = False
    return bool((buf[mask] == fill).all())


def _scratch(torch, L, level, lens, decode):
    arr = (ctypes.c_uint64 * max(len(lens), 1))(*lens)
    need = L.chipx_ragged_scratch_len(level, arr, len(lens), int(decode))
    return torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda"), need


def _encode_and_check(gpu, level, sizes, stream_offset):
    import torch
    from carbonado_amd import device as D
    host, in_off = _pack([_data(n) for n in sizes])
    inp = torch.from_numpy(host).cuda()
    out_off, lay_len, total = D.ragged_layout(level, sizes, align=256, stream_offset=stream_offset)
    out = torch.full((total + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    hashes = torch.full((len(sizes), 32), 0xA5, dtype=torch.uint8, device="cuda")
    scratch, need = _scratch(torch, gpu, level, sizes, False)
    out_len, infos = D.encode_ragged(level, inp, in_off, sizes, out, out_off, hashes, scratch)
    torch.cuda.synchronize()
    got, gh = out.cpu().numpy(), hashes.cpu().numpy()
    assert out_len == lay_len
    for i, n in enumerate(sizes):
        enc, h, info = _oracle(n, level)
        assert out_len[i] == len(enc), (level, n)
        assert got[out_off[i]:out_off[i] + len(enc)].tobytes() == enc, (level, n, stream_offset)
        assert gh[i].tobytes() == h, (level, n)
        _check_info(infos[i], info, (level, n))
        if level & 4:
            assert out_off[i] % 256 == stream_offset
    assert _untouched(got, out_off, out_len), "bytes outside the objects' output ranges were written"
    assert bool((scratch[need:] == 0xA5).all()), "scratch written past chipx_ragged_scratch_len"
    return got, out_off, out_len


def _shuffled(seed):
    return [SIZES[i] for i in np.random.default_rng(seed).permutation(len(SIZES))]


@pytest.mark.parametrize("level", LEVELS)
def test_ragged_encode_matches_oracle(gpu, level):
    sizes = _shuffled(11)
    _encode_and_check(gpu, level, sizes, 56)
    _encode_and_check(gpu, level, sizes, 0)
    if level & 4:
        _encode_and_check(gpu, level, sizes, 8)


def _decode_and_check(gpu, level, sizes, stream_offset=56):
    import torch
    from carbonado_amd import device as D
    encs = [_oracle(n, level) for n in sizes]
    in_off, in_len, total = D.ragged_layout(level, sizes, align=256, stream_offset=stream_offset)
    host = np.full(total + 256, 0x5A, dtype=np.uint8)
    for o, (enc, _, _) in zip(in_off, encs):
        host[o:o + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    enc_d = torch.from_numpy(host).cuda()
    hashes = torch.from_numpy(np.frombuffer(b"".join(h for _, h, _ in encs), dtype=np.uint8).copy()).cuda()
    padding = [info["padding_len"] for _, _, info in encs]
    exp, out_off = _pack([_data(n) for n in sizes], fill=0xA5)
    out = torch.full((exp.size,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((len(sizes),), 77, dtype=torch.int32, device="cuda")
    scratch, need = _scratch(torch, gpu, level, in_len, True)
    out_len = D.decode_ragged(level, enc_d, in_off, in_len, hashes, padding, out, out_off, status, scratch)
    torch.cuda.synchronize()
    assert out_len == list(sizes)
    assert status.cpu().tolist() == [0] * len(sizes)
    assert np.array_equal(out.cpu().numpy(), exp), "content differs, or bytes outside the ranges were written"
    assert bool((scratch[need:] == 0xA5).all())


@pytest.mark.parametrize("level", LEVELS)
def test_ragged_decode_round_trip(gpu, level):
    sizes = _shuffled(11)
    for n in sizes:  # the oracle's own round trip of what is decoded below
        enc, h, info = _oracle(n, level)
        assert O.decode(h, enc, info["padding_len"], level) == _data(n)
    _decode_and_check(gpu, level, sizes)


# ---- damage --------------------------------------------------------------

def _ceil_log2(x):
    return 0 if x <= 1 else (x - 1).bit_length()


def _spots(bao_n):
    """name -> byte offset in a stream of bao_n content bytes (None: no such node)"""
    N = max(1, (bao_n + 1023) // 1024)
    root_level = _ceil_log2(N)
    return {
        "header": 3,
        "root": 8 + 17 if N > 1 else None,
        "chunk0": chunk_off(0, N) if bao_n else None,
        "last_chunk": 8 + bao_n + 64 * (N - 1) - 1 if bao_n else None,
        "level1_group0": chunk_off(0, N) - 64 + 40 if N > 1 else None,
        # the level-7 node over groups 0 and 1 on the left spine, where it is not the root itself
        "above_groups": 8 + 64 * (root_level - 7) + 33 if root_level > 7 else None,
        "hash": -1,
    }


DAMAGE_SIZES = [1, 4097, 32769, 65537, 200001, 1 << 20, 1024, 66560]


@pytest.mark.parametrize("level", [4, 12])
def test_ragged_decode_isolates_damage(gpu, level):
    import torch
    from carbonado_amd import device as D
    sizes = DAMAGE_SIZES
    encs = [_oracle(n, level) for n in sizes]
    in_off, in_len, total = D.ragged_layout(level, sizes)
    host = np.full(total + 256, 0x5A, dtype=np.uint8)
    for o, (enc, _, _) in zip(in_off, encs):
        host[o:o + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
    enc_d = torch.from_numpy(host).cuda()
    hashes = torch.from_numpy(np.frombuffer(b"".join(h for _, h, _ in encs), dtype=np.uint8).copy()).cuda()
    hashes = hashes.view(len(sizes), 32)
    padding = [info["padding_len"] for _, _, info in encs]
    exp_h, out_off = _pack([_data(n) for n in sizes], fill=0xA5)
    exp = torch.from_numpy(exp_h).cuda()
    out = torch.empty_like(exp)
    status = torch.empty((len(sizes),), dtype=torch.int32, device="cuda")
    scratch = D.ragged_scratch(level, in_len, decode=True)
    bao_n = [8 * info["chunk_len"] if level & 8 else n for n, (_, _, info) in zip(sizes, encs)]
    hit = {}
    for o, n in enumerate(sizes):
        multi = (bao_n[o] + 1023) // 1024 > 64
        for name, pos in _spots(bao_n[o]).items():
            if pos is None:
                continue
            target = hashes[o] if name == "hash" else enc_d[in_off[o]:in_off[o] + in_len[o]]
            idx = 9 if name == "hash" else pos
            target[idx] ^= 0x10
            out.fill_(0xA5)
            status.fill_(77)
            D.decode_ragged(level, enc_d, in_off, in_len, hashes, padding, out, out_off, status, scratch)
            bad = torch.nonzero(out != exp).flatten()
            st = status.cpu().tolist()
            target[idx] ^= 0x10
            assert st == [5 if i == o else 0 for i in range(len(sizes))], (level, n, name, st)
            if bad.numel():  # only the damaged object's own content may differ
                lo, hi = int(bad.min()), int(bad.max())
                assert out_off[o] <= lo and hi < out_off[o] + sizes[o], (level, n, name, lo, hi)
            hit.setdefault(name, set()).add(multi)
    for name in ("header", "root", "chunk0", "last_chunk", "level1_group0", "hash"):
        assert hit[name] == {True, False}, (name, hit[name])
    assert hit["above_groups"] == {True}  # a single-group object has no node above its group


# ---- against the uniform batch -------------------------------------------

def test_ragged_equals_uniform_batch(gpu):
    import torch
    from carbonado_amd import device as D
    n, count = 300001, 5
    datas = [np.random.default_rng(50 + i).integers(0, 256, n, dtype=np.uint8).tobytes() for i in range(count)]
    for level in (4, 12):
        # the uniform call wants 16-B aligned rows where its small-object kernels write them (level 4 here)
        so = 56 if level == 12 else 0
        host, in_off = _pack(datas)
        inp = torch.from_numpy(host).cuda()
        out_off, lay_len, total = D.ragged_layout(level, [n] * count, stream_offset=so)
        out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        hashes = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        D.encode_ragged(level, inp, in_off, [n] * count, out, out_off, hashes, D.ragged_scratch(level, [n] * count))
        pitch = total // count  # equal lengths: the layout's rows are a uniform batch's rows
        assert out_off == [so + i * pitch for i in range(count)]
        uin = torch.from_numpy(np.stack([np.frombuffer(d, dtype=np.uint8) for d in datas])).cuda()
        uin = torch.nn.functional.pad(uin, (0, 15))[:, :(n + 15) // 16 * 16].contiguous()
        uout = torch.full((count, pitch), 0xA5, dtype=torch.uint8, device="cuda")
        uh = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        ulen, _ = D.encode_batch(level, uin, n, uout, uh, D.encode_scratch(level, n, count), out_offset=so)
        torch.cuda.synchronize()
        assert ulen == lay_len[0]
        assert torch.equal(out.view(count, pitch)[:, so:so + ulen], uout[:, so:so + ulen])
        assert torch.equal(hashes, uh)
        dec = torch.zeros((count, (n + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
        st = torch.full((count,), 77, dtype=torch.int32, device="cuda")
        pad = _pad_of(level, n)
        dlen = D.decode_batch(level, out.view(count, pitch), ulen, hashes, pad, dec, st,
                              D.decode_scratch(level, ulen, count), in_offset=so)
        torch.cuda.synchronize()
        assert dlen == n and st.cpu().tolist() == [0] * count
        assert torch.equal(dec[:, :n], uin[:, :n])


def _pad_of(level, n):
    return (-n) % 4096 if level & 8 else 0


def test_ragged_back_to_back(gpu):
    """Six calls on one stream without a synchronise between them, sharing one
    scratch: descriptor tables, group CVs and scratch reuse are stream-ordered."""
    import torch
    from carbonado_amd import device as D
    comps = [(4, [65537]), (12, [200001, 1]), (4, _shuffled(3)), (12, _shuffled(4)), (4, [1025, 0, 66560]),
             (12, [32769, 4097, 32768, 65])]
    assert [len(c[1]) for c in comps][:4] == [1, 2, 27, 27]
    need = 0
    for level, sizes in comps:
        need = max(need, gpu.chipx_ragged_scratch_len(level, (ctypes.c_uint64 * len(sizes))(*sizes), len(sizes), 0))
    scratch = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    jobs = []
    for level, sizes in comps:
        host, in_off = _pack([_data(n) for n in sizes])
        out_off, lay_len, total = D.ragged_layout(level, sizes)
        jobs.append((level, sizes, torch.from_numpy(host).cuda(), in_off, out_off, lay_len,
                     torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda"),
                     torch.zeros((len(sizes), 32), dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for level, sizes, inp, in_off, out_off, _, out, hashes in jobs:
            D.encode_ragged(level, inp, in_off, sizes, out, out_off, hashes, scratch)
    s.synchronize()
    for level, sizes, _, _, out_off, lay_len, out, hashes in jobs:
        got, gh = out.cpu().numpy(), hashes.cpu().numpy()
        for i, n in enumerate(sizes):
            enc, h, _ = _oracle(n, level)
            assert got[out_off[i]:out_off[i] + len(enc)].tobytes() == enc, (level, n)
            assert gh[i].tobytes() == h
        assert _untouched(got, out_off, lay_len)
    assert bool((scratch[need:] == 0xA5).all())


def test_ragged_largest_object(gpu):
    import torch
    from carbonado_amd import device as D
    from carbonado_amd.error import InvalidArgument
    sizes = [1, 16 << 20, 4097]
    got, out_off, out_len = _encode_and_check(gpu, 12, sizes, 56)
    _decode_and_check(gpu, 12, sizes)
    # one byte over the limit: rejected on the host, nothing written
    sizes = [1, (16 << 20) + 1, 4097]
    inp = torch.zeros(((16 << 20) + 64,), dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    hashes = torch.full((3, 32), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(InvalidArgument):
        D.encode_ragged(12, inp, [0, 16, 32], sizes, out, [56, 1024, 2048], hashes, torch.zeros(8192, dtype=torch.uint8,
                                                                                                   device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((hashes == 0xA5).all())


@pytest.mark.parametrize("level", LEVELS)
def test_ragged_seeded_random(gpu, level):
    rng = np.random.default_rng(2024)
    sizes = [int(round(math.exp(x))) for x in rng.uniform(0.0, math.log(2 << 20), 64)]
    assert min(sizes) >= 1 and max(sizes) <= 2 << 20
    _encode_and_check(gpu, level, sizes, 56)
    _decode_and_check(gpu, level, sizes)
