"""CPU tests of the audit boundary (include/carbonado_hip_audit.h): the
chipa_* symbols, their ctypes and Rust bindings, the host-only layout against
the oracle's slices, the argument errors an audit call decides before it
touches a device, and the host logic and item-to-node arithmetic behind them
as a stand-alone program under ASan + UBSan."""
import ctypes
import random
import re
from pathlib import Path

import pytest

import boundary as B
import test_rust_shim as RS
from test_slice_verify import _grid
from carbonado_amd import _lib
from oracle import oracle as O
from oracle import pyoracle as P

ROOT = Path(__file__).resolve().parents[1]
AUDIT_HEADER = ROOT / "include" / "carbonado_hip_audit.h"
FFI_AUDIT = ROOT / "carbonado-hip" / "src" / "ffi_audit.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

SIZES = [0, 1, 1023, 1024, 1025, 2049, 3072, 5121, 8193, 66561, (1 << 20) + 5]
OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100


def audit_prototypes() -> dict:
    return B.prototypes(AUDIT_HEADER, "chipa_")


def test_audit_exports_header_and_ctypes_are_one_set():
    protos = audit_prototypes()
    assert len(protos) == 6
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipa_")
    assert _lib.lib().chipa_abi_version() == 1
    assert "#define CHIPA_ABI_VERSION 1" in AUDIT_HEADER.read_text()
    # the two older boundaries keep their sets
    B.assert_older_keep_their_sets(exported, "chipa_")


def test_ffi_audit_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI_AUDIT, "chipa_"), audit_prototypes())
    text = B.ffi_text(FFI_AUDIT)
    assert re.search(r"pub const CHIPA_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_audit;", lib, flags=re.M)
    for fn, call in (("extract_slices", "chipa_extract_slices_dev"), ("verify_slices", "chipa_verify_slices_dev"),
                     ("verify_slice_proofs", "chipa_verify_proofs_dev")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_audit::{call}(" in body, fn
        assert "DeviceBuffer" in body.split("{", 1)[0]


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


def _u32(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def _layout(ns, index, count, align=16):
    k = len(ns)
    outs = [_u64([0] * k) for _ in range(4)]
    pt, ct = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _lib.lib().chipa_slice_layout(_u64(ns), _u64(index), _u64(count), k, align, *outs, ctypes.byref(pt),
                                       ctypes.byref(ct))
    return rc, [list(o)[:k] for o in outs], pt.value, ct.value


@pytest.fixture(scope="module")
def streams():
    """n -> (content, stream, hash), each encoded once"""
    out = {}
    for n in SIZES:
        d = random.Random(n).randbytes(n)
        enc, h = O.bao_encode(d)
        out[n] = (d, enc, h)
    return out


@pytest.mark.parametrize("align", [16, 256])
def test_slice_layout_matches_the_oracle(streams, align):
    L = _lib.lib()
    ns, index, count = [], [], []
    for n in SIZES:
        for i, c in _grid(n):
            ns.append(n); index.append(i); count.append(c)
    rc, (poff, plen, coff, clen), pt, ct = _layout(ns, index, count, align)
    assert rc == OK
    for r, (n, i, c) in enumerate(zip(ns, index, count)):
        start, length = i * 1024, c * 1024
        assert plen[r] == len(P.bao_slice(streams[n][1], start, length)) == L.chip_bao_slice_len(n, start, length)
        assert clen[r] == (min(n, start + length) - start if start < n else 0) == len(streams[n][0][start:start + length])
        assert poff[r] % align == 0 and coff[r] % align == 0
    up = lambda x: -(-x // align) * align  # noqa: E731
    for off, ln, total in ((poff, plen, pt), (coff, clen, ct)):
        rows = sorted((o, o + x) for o, x in zip(off, ln) if x)
        assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:])), "ranges overlap"
        assert total == sum(up(x) for x in ln) == up(rows[-1][1])  # tight: the rounded lengths and nothing more
    assert _layout(ns, index, count, 8)[0] == INVALID_ARG
    assert _layout(ns, index, count, 0)[0] == INVALID_ARG
    assert _layout([5000], [(1 << 53) + 1], [1])[0] == INVALID_ARG
    last = len(P.bao_slice(O.bao_encode(bytes(5000))[0], 1 << 63, 1 << 63))  # start + len = 2^64: no wrap
    assert _layout([5000], [1 << 53], [1 << 53])[:2] == (OK, [[0], [last], [0], [0]])
    assert _layout([5000], [0], [1 << 53])[1][3] == [5000]
    assert _layout([], [], [])[0] == OK


# never dereferenced: the checks come first
STR, PRF, CNT, HASH, STAT, SCR = 0x10000000, 0x40000000, 0x50000000, 0x70000000, 0x74000000, 0x78000000
N2 = [5000, 70000]
LEN2 = [8 + n + 64 * (-(-n // 1024) - 1) for n in N2]
OFF2 = [56, 1 << 20]


def _extract(req_stream=(0, 1, 1), index=(0, 3, 68), count=(1, 2, 0), in_off=OFF2, in_len=LEN2, proof_off=None,
             proof_len=None, nreq=None, streams=STR, proofs=PRF, scratch=SCR, arrays=True):
    ns = [N2[s] if s < 2 else 0 for s in req_stream]
    _, (poff, plen, _, _), _, _ = _layout(ns, list(index), list(count))
    poff = list(proof_off) if proof_off is not None else poff
    plen = list(proof_len) if proof_len is not None else plen
    nreq = len(req_stream) if nreq is None else nreq
    return _lib.lib().chipa_extract_slices_dev(streams, _u64(in_off), _u64(in_len), len(in_len), _u32(req_stream),
                                               _u64(index) if arrays else None, _u64(count), nreq, proofs, _u64(poff),
                                               _u64(plen), scratch, None)


def _verify(req_stream=(0, 1, 1), index=(0, 3, 68), count=(1, 2, 0), in_off=OFF2, in_len=LEN2, content_off=None,
            nreq=None, hashes=HASH, status=STAT, arrays=True):
    ns = [N2[s] if s < 2 else 0 for s in req_stream]
    _, (_, _, coff, _), _, _ = _layout(ns, list(index), list(count))
    coff = list(content_off) if content_off is not None else coff
    nreq = len(req_stream) if nreq is None else nreq
    return _lib.lib().chipa_verify_slices_dev(STR, _u64(in_off), _u64(in_len), hashes, len(in_len), _u32(req_stream),
                                              _u64(index), _u64(count) if arrays else None, nreq, CNT, _u64(coff),
                                              _u64([0] * len(req_stream)), status, SCR, None)


def _proofs(index=(0, 3, 68), count=(1, 2, 0), ns=(5000, 70000, 70000), proof_off=None, proof_len=None,
            content_off=None, nreq=None, hashes=HASH, arrays=True):
    _, (poff, plen, coff, _), _, _ = _layout(list(ns), list(index), list(count))
    poff = list(proof_off) if proof_off is not None else poff
    plen = list(proof_len) if proof_len is not None else plen
    coff = list(content_off) if content_off is not None else coff
    nreq = len(ns) if nreq is None else nreq
    return _lib.lib().chipa_verify_proofs_dev(PRF, _u64(poff), _u64(plen), _u64(ns) if arrays else None, hashes,
                                              _u64(index), _u64(count), nreq, CNT, _u64(coff), _u64([0] * len(ns)),
                                              STAT, SCR, None)


def test_audit_argument_errors_need_no_device():
    big = (1 << 53) + 1
    # NULL arrays or buffers with nreq > 0
    assert _extract(arrays=False) == INVALID_ARG and _verify(arrays=False) == INVALID_ARG
    assert _proofs(arrays=False) == INVALID_ARG
    assert _extract(streams=None) == INVALID_ARG and _extract(proofs=None) == INVALID_ARG
    assert _extract(scratch=None) == INVALID_ARG and _verify(status=None) == INVALID_ARG
    # a request on a stream that is not there; index or count above 2^53
    assert _extract(req_stream=(0, 2, 1)) == INVALID_ARG and _verify(req_stream=(0, 2, 1)) == INVALID_ARG
    for f in (_extract, _verify, _proofs):
        assert f(index=(0, big, 68)) == INVALID_ARG, f
        assert f(count=(1, 2, big)) == INVALID_ARG, f
    # stream and proof addresses want 8, content addresses 16
    assert _extract(in_off=[60, 1 << 20]) == INVALID_ARG and _verify(in_off=[56, (1 << 20) + 4]) == INVALID_ARG
    assert _extract(proof_off=[0, 4100, 8192]) == INVALID_ARG and _proofs(proof_off=[0, 4100, 8192]) == INVALID_ARG
    assert _verify(content_off=[0, 1032, 4096]) == INVALID_ARG and _proofs(content_off=[0, 1032, 4096]) == INVALID_ARG
    # overlapping output ranges, in either order
    assert _extract(proof_off=[0, 1024, 8192]) == INVALID_ARG and _extract(proof_off=[1024, 0, 8192]) == INVALID_ARG
    assert _verify(content_off=[0, 512, 8192]) == INVALID_ARG and _proofs(content_off=[512, 0, 8192]) == INVALID_ARG
    # no bao stream has that length; a proof of the wrong length
    gap = 8 + 5120 + 64 * 4 + 16  # between the streams of 5120 and 5121 bytes (one more chunk: 65 bytes on)
    assert _extract(in_len=[gap, LEN2[1]]) == TRUNCATED and _verify(in_len=[LEN2[0], 7]) == TRUNCATED
    assert _verify(in_len=[gap, LEN2[1]]) == TRUNCATED
    good = _layout([5000, 70000, 70000], [0, 3, 68], [1, 2, 0])[1][1]
    assert _extract(proof_len=[good[0], good[1] - 64, good[2]]) == TRUNCATED
    assert _proofs(proof_len=[good[0], good[1], good[2] - 8]) == TRUNCATED
    # INVALID_ARG before BAO_TRUNCATED before HASH_DECODE
    assert _verify(in_len=[gap, LEN2[1]], content_off=[0, 1032, 4096]) == INVALID_ARG
    assert _verify(hashes=None) == HASH_DECODE and _proofs(hashes=None) == HASH_DECODE
    assert _verify(hashes=None, in_len=[gap, LEN2[1]]) == TRUNCATED
    # nothing to do
    assert _extract(nreq=0) == OK and _verify(nreq=0) == OK and _proofs(nreq=0) == OK
    assert _extract(nreq=0, arrays=False, streams=None, proofs=None, scratch=None) == OK
    # a well-formed call gets as far as the device and no further
    import torch
    if not torch.cuda.is_available():
        assert _extract() == NO_DEVICE and _verify() == NO_DEVICE and _proofs() == NO_DEVICE


def test_audit_scratch_len_covers_the_table():
    L = _lib.lib()
    for nreq in (0, 1, 3, 1000, 12544):
        need = 64 * nreq + 3 * 8 * (nreq + 1)
        got = L.chipa_audit_scratch_len(7, nreq)
        assert need <= got <= need + 4 * 256 + 16 and got % 16 == 0
        assert got == L.chipa_audit_scratch_len(1 << 20, nreq)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "audit_plan_check.cpp")


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_audit_plan_under_asan_ubsan(plan_check, seed):
    """Checks, layout, request table and prefix arrays of an audit call are
    host code (audit_plan.hpp): a stand-alone program drives them over seeded
    mixes, and checks that every request's work items tile its proof."""
    assert "0 failures" in B.run_check(plan_check, "plan", seed)


@pytest.mark.parametrize("n", SIZES)
def test_work_items_are_the_nodes_bao_slice_selects(plan_check, streams, n):
    """Every request's work items, enumerated by the arithmetic the kernels
    compile (audit_nodes.hpp): the bytes at their stream offsets, put at their
    proof offsets, are the oracle's slice; and the 32 bytes each node is to be
    compared with are that node's chaining value, at the stream address and
    at the proof address alike (the memo of a clean stream holds every CV)."""
    _, enc, h = streams[n]
    memo = P.bao_prime(enc, h)
    grid = _grid(n)
    out = B.run_check(plan_check, "nodes", *[str(x) for i, c in grid for x in (n, i, c)])
    reqs = []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "req":
            reqs.append(([int(x) for x in f[1:]], []))
        else:
            reqs[-1][1].append((f[1], *[int(x) for x in f[2:]]))
    assert len(reqs) == len(grid)
    for (i, c), (head, nodes) in zip(grid, reqs):
        assert head[:3] == [n, i, c]
        want = P.bao_slice(enc, i * 1024, c * 1024)
        assert head[7] == len(want), (n, i, c)
        proof = bytearray(len(want))
        proof[:8] = enc[:8]
        covered = 8
        for kind, level, s, soff, size, poff, slot_s, slot_p in nodes:
            proof[poff:poff + size] = enc[soff:soff + size]
            covered += size
        assert covered == len(want) and bytes(proof) == want, (n, i, c)
        for kind, level, s, soff, size, poff, slot_s, slot_p in nodes:
            data = enc[soff:soff + size]
            if slot_s < 0:  # the root: compared with the hash
                assert memo[("parent_root" if kind == "P" else "chunk_root", 0 if kind == "P" else s, data)] == h
                continue
            cv = memo[("parent" if kind == "P" else "chunk", 0 if kind == "P" else s, data)]
            assert enc[slot_s:slot_s + 32] == cv == bytes(proof[slot_p:slot_p + 32]), (n, i, c, kind, level, s)
