"""The Python oracle's bao slice verifier (pyoracle.bao_decode_slice, a
restatement of bao's SliceDecoder) pinned down without a device, so that the
scrub / verify_slice GPU tests can take their verdicts from it: clean slices
return the content, the whole-stream slice agrees with the C oracle's
bao_decode, and for every single damaged node the authentic shards equal a
closed form written separately (tests/bao_damage.py: bottom-up tree, "the
shards whose chunk range misses the node's subtree")."""
import random

import pytest

import bao_damage as B  # tests/bao_damage.py (tests/ is on sys.path under pytest)
from carbonado_amd import decoding
from oracle import oracle as O
from oracle import pyoracle as P

SIZES = [0, 1, 1024, 1025, 3000, 5121, 8193, 66561]


def _grid(n):
    N = max(1, -(-n // 1024))
    idx = sorted({0, 1, 2, N // 2, N - 2, N - 1, N, N + 2} & set(range(N + 3)))
    cnt = sorted({0, 1, 2, 3, N // 2, N - 1, N, N + 1} & set(range(N + 2)))
    return [(i, c) for i in idx for c in cnt]


@pytest.mark.parametrize("n", SIZES)
def test_clean_slices_return_the_content(n):
    d = random.Random(n).randbytes(n)
    enc, h = O.bao_encode(d)
    memo = P.bao_prime(enc, h)
    grid = _grid(n)
    assert {(0, 0), (max(1, -(-n // 1024)) + 2, 1)} <= set(grid)
    for index, count in grid:
        start, length = index * 1024, count * 1024
        sl = P.bao_slice(enc, start, length)
        assert P.bao_decode_slice(sl, h, start, length, memo) == d[start:start + length], (n, index, count)
    # byte ranges that are no multiple of a chunk, and the memo changes nothing
    for start, length in [(0, 1), (1, 1), (1023, 2), (1500, 3000), (n - 1 if n else 0, 5), (n, 1), (n + 5000, 7)]:
        sl = P.bao_slice(enc, start, length)
        assert P.bao_decode_slice(sl, h, start, length, memo) == d[start:start + length], (n, start, length)
        if n <= 8193:
            assert P.bao_decode_slice(sl, h, start, length) == d[start:start + length], (n, start, length)


@pytest.mark.parametrize("n", [0, 1, 1024, 1025, 3000, 5121])
def test_whole_stream_verdict_is_bao_decode(n):
    """The slice of everything is the stream itself, and the verifier (hashing
    for real, no memo) accepts it exactly when the C oracle's bao_decode does:
    clean, every node damaged in turn, the header, the hash, a cut-off stream."""
    d = random.Random(100 + n).randbytes(n)
    enc, h = O.bao_encode(d)
    assert P.bao_slice(enc, 0, n) == enc
    rng = random.Random(n)
    nodes = B.tree_nodes(n)
    streams = [(enc, h)]
    streams += [(B.flip(enc, nodes, c, rng), h) for c in B.every_node_cases(nodes) if nodes[c[0]].size]
    for bit in (0, 3, 10, 13, 40):
        b = bytearray(enc)
        b[bit // 8] ^= 1 << bit % 8
        streams.append((bytes(b), h))
    streams.append((enc, bytes([h[0] ^ 1]) + h[1:]))
    streams += [(enc[:len(enc) - 1], h), (enc[:8], h)] if n else []
    accepted = 0
    for s, hh in streams:
        try:
            want = O.bao_decode(s, hh)
        except O.OracleError:
            want = None
        try:
            got = P.bao_decode_slice(P.bao_slice(s, 0, n), hh, 0, n)
        except P.SliceError:
            got = None
        assert got == want, (n, s[:8].hex())
        accepted += want is not None
    assert accepted == 1  # only the clean stream


@pytest.mark.parametrize("spc", [1, 3, 13])
def test_every_damaged_node_spoils_the_shards_it_covers(spc):
    N = 8 * spc
    d = random.Random(spc).randbytes(N * 1024)
    enc, h = O.bao_encode(d)
    memo = P.bao_prime(enc, h)
    nodes = B.tree_nodes(len(d))
    assert len(nodes) == 2 * N - 1 and nodes[-1].off + nodes[-1].size == len(enc)
    cases = B.every_node_cases(nodes)
    assert len(cases) == 2 * (N - 1) + N
    assert P.authentic_shards(enc, h, spc, memo) == set(range(8))
    rng = random.Random(N)
    for case in cases:
        bad = B.flip(enc, nodes, case, rng)
        assert P.authentic_shards(bad, h, spc, memo) == B.shards_missing(nodes[case[0]], spc), (spc, case)


def test_memo_does_not_change_a_verdict():
    d = random.Random(5).randbytes(8192)
    enc, h = O.bao_encode(d)
    memo = P.bao_prime(enc, h)
    nodes = B.tree_nodes(len(d))
    rng = random.Random(6)
    for case in B.every_node_cases(nodes):
        bad = B.flip(enc, nodes, case, rng)
        assert P.authentic_shards(bad, h, 1) == P.authentic_shards(bad, h, 1, memo), case


def test_prime_refuses_a_stream_that_does_not_verify():
    enc, h = O.bao_encode(random.Random(7).randbytes(3000))
    with pytest.raises(O.OracleError):
        P.bao_prime(enc[:100] + bytes([enc[100] ^ 1]) + enc[101:], h)


@pytest.mark.parametrize("n", SIZES)
def test_extracted_slices_verify(n):
    """chip_bao_extract_slice (byte selection, no device) hands out slices the
    verifier accepts, and they hold the content asked for."""
    d = random.Random(n).randbytes(n)
    enc, h = O.bao_encode(d)
    memo = P.bao_prime(enc, h)
    N = max(1, -(-n // 1024))
    for index in sorted({0, 1, N // 2, N - 1, N, N + 3}):
        for slen in (0, 1, 1024, 1500, 4096, N * 1024):
            got = decoding.extract_slice(enc, index, slen)
            start = index * 1024
            assert P.bao_decode_slice(got, h, start, slen, memo) == d[start:start + slen], (n, index, slen)
