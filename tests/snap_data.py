"""Inputs and stream tools shared by the snappy device tests: the seeded mix
of random runs and repeats, the object set, a walker that names what a frame
stream contains (so a test can require that its inputs exercise every kind of
chunk, tag and header before it compares anything), and hand-built streams."""
import functools
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
SAMPLES = ROOT / "tests" / "golden" / "samples"

LENGTHS = [0, 1, 16, 17, 18, 255, 256, 257, 512, 513, 4096, 4097, 16384, 16385, 65535, 65536, 65537, 131073, 200000]
REPEATS = [4, 5, 7, 11, 12, 20, 59, 60, 61, 64, 65, 67, 68, 69, 130, 300]
STREAM_ID = b"\xff\x06\x00\x00sNaPpY"
BLOCK = 65536


def mix(n: int, L: int, seed: int) -> bytes:
    """Random runs of 1..L bytes alternating with repeats of earlier output:
    lengths from REPEATS, offsets from 1-8, 9-2047 and 2048-65535."""
    rng = np.random.default_rng(seed)
    v = bytearray()
    while len(v) < n:
        v += rng.integers(0, 256, int(rng.integers(1, L + 1)), dtype=np.uint8).tobytes()
        ln = REPEATS[int(rng.integers(0, len(REPEATS)))]
        lo, hi = ((1, 9), (9, 2048), (2048, 65536))[int(rng.integers(0, 3))]
        off = min(int(rng.integers(lo, hi)), len(v))
        if off >= ln:
            v += v[len(v) - off:len(v) - off + ln]
        else:  # an overlapping repeat: the pattern of `off` bytes, again and again
            pat = bytes(v[len(v) - off:])
            v += (pat * (ln // off + 1))[:ln]
    return bytes(v[:n])


@functools.lru_cache(maxsize=None)
def objects():
    """About 60 objects as (name, bytes): random, zero, the sample files, and
    the mixes.  L = 40 compresses in every block; L = 300 and L = 400 over two
    blocks sit across FrameEncoder's 1/8 rule."""
    rng = np.random.default_rng(2024)
    objs = [(f"random{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in LENGTHS]
    objs += [(f"zeros{n}", bytes(n)) for n in (1, 17, 257, 4097, 65536, 65537, 200000)]
    objs += [(p.name, p.read_bytes()) for p in sorted(SAMPLES.iterdir())]
    objs += [(f"mix40_{n}", mix(n, 40, 100 + i)) for i, n in enumerate(LENGTHS) if n >= 17]
    objs += [(f"mix300_{s}", mix(2 * BLOCK, 300, s)) for s in (300, 301, 302, 303)]
    objs += [(f"mix400_{s}", mix(2 * BLOCK, 400, s)) for s in (400, 401, 402, 403)]
    return objs


def chunks(stream: bytes):
    """(type, body) of every chunk of a frame stream."""
    s, out = 0, []
    while s < len(stream):
        n = int.from_bytes(stream[s + 1:s + 4], "little")
        out.append((stream[s], stream[s + 4:s + 4 + n]))
        s += 4 + n
    assert s == len(stream)
    return out


def kinds(stream: bytes) -> set:
    """What a frame stream contains: 'raw', 'compressed', and per tag of its
    compressed chunks 'copy1', 'copy2', 'copy4', 'len60', 'len64', 'far'
    (offset >= 32768), 'overlap' (offset < length), 'lit1' .. 'lit5' (bytes of
    the literal header)."""
    found = set()
    for ty, body in chunks(stream):
        if ty == 1:
            found.add("raw")
        if ty != 0:
            continue
        found.add("compressed")
        b, s = body[4:], 0
        while b[s] & 0x80:
            s += 1
        s += 1
        while s < len(b):
            tag = b[s]
            if tag & 3 == 0:
                x = tag >> 2
                nb = x - 59 if x >= 60 else 0
                if nb:
                    x = int.from_bytes(b[s + 1:s + 1 + nb], "little")
                found.add(f"lit{1 + nb}")
                s += 1 + nb + x + 1
                continue
            if tag & 3 == 1:
                ln, off, s = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | b[s + 1], s + 2
                found.add("copy1")
            elif tag & 3 == 2:
                ln, off, s = 1 + (tag >> 2), int.from_bytes(b[s + 1:s + 3], "little"), s + 3
                found.add("copy2")
            else:
                ln, off, s = 1 + (tag >> 2), int.from_bytes(b[s + 1:s + 5], "little"), s + 5
                found.add("copy4")
            if ln in (60, 64):
                found.add(f"len{ln}")
            if off >= 32768:
                found.add("far")
            if off < ln:
                found.add("overlap")
    return found


# ---- hand-built streams ------------------------------------------------------
def crc_masked(data: bytes) -> int:
    from oracle import host_oracle as H
    return H.crc32c_masked(bytes(data))


def chunk(ty: int, body: bytes) -> bytes:
    return bytes([ty]) + len(body).to_bytes(3, "little") + body


def data_chunk(content: bytes, body: bytes = None, crc: int = None) -> bytes:
    """A data chunk for `content`: raw, or compressed with the given snappy
    body (varint included)."""
    word = (crc_masked(content) if crc is None else crc).to_bytes(4, "little")
    return chunk(0x01, word + content) if body is None else chunk(0x00, word + body)


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def literal(data: bytes, header_bytes: int = 0) -> bytes:
    """A literal element; header_bytes = 2..5 forces a longer header than needed."""
    n = len(data) - 1
    if header_bytes == 0:
        header_bytes = 1 if n < 60 else 2 if n < 256 else 3
    if header_bytes == 1:
        return bytes([n << 2]) + data
    nb = header_bytes - 1
    return bytes([(59 + nb) << 2]) + n.to_bytes(nb, "little") + data


def copy1(off: int, ln: int) -> bytes:
    return bytes([((off >> 8) << 5) | ((ln - 4) << 2) | 1, off & 255])


def copy2(off: int, ln: int) -> bytes:
    return bytes([((ln - 1) << 2) | 2]) + off.to_bytes(2, "little")


def copy4(off: int, ln: int) -> bytes:
    return bytes([((ln - 1) << 2) | 3]) + off.to_bytes(4, "little")


def expand(pattern: bytes, ln: int) -> bytes:
    """What a copy of `ln` bytes at offset len(pattern) appends."""
    return (pattern * (ln // len(pattern) + 1))[:ln]
