"""CPU tests of the read boundary (include/carbonado_hip_read.h): the chipd_*
symbols, their ctypes and Rust bindings, the argument errors a ranged read
decides before it touches a device, in their stated order, the layout against
plain arithmetic, and the host logic behind them
(carbonado_amd/csrc/read_plan.hpp) as a stand-alone program under ASan +
UBSan."""
import ctypes
import random
import re
from pathlib import Path

import pytest

import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
READ_HEADER = ROOT / "include" / "carbonado_hip_read.h"
FFI_READ = ROOT / "carbonado-hip" / "src" / "ffi_read.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100


def read_prototypes() -> dict:
    return B.prototypes(READ_HEADER, "chipd_")


def test_read_exports_header_and_ctypes_are_one_set():
    protos = read_prototypes()
    assert len(protos) == 4
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipd_")
    assert _lib.lib().chipd_abi_version() == 1
    assert "#define CHIPD_ABI_VERSION 1" in READ_HEADER.read_text()
    # the four older boundaries keep their sets
    B.assert_older_keep_their_sets(exported, "chipd_")


def test_ffi_read_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI_READ, "chipd_"), read_prototypes())
    text = B.ffi_text(FFI_READ)
    assert re.search(r"pub const CHIPD_ABI_VERSION: c_int = 1;", text)


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_read;", lib, flags=re.M)
    for fn, call in (("read_layout", "chipd_read_layout"), ("read_scratch_len", "chipd_read_scratch_len"),
                     ("read_ranges", "chipd_read_ranges_dev")):
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert f"ffi_read::{call}(" in body, fn
    m = re.search(r"\npub fn read_ranges\(", lib)
    assert "DeviceBuffer" in lib[m.end():].split("{", 1)[0]


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


def _u32(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def _blen(n):
    return 8 + n + 64 * (max(1, -(-n // 1024)) - 1)


# never dereferenced: the checks come first
STR, OUT, HASH, STAT, USED, SCR = 0x10000000, 0x40000000, 0x70000000, 0x74000000, 0x76000000, 0x78000000
SPC = [1, 5, 9]
LEN3 = [_blen(8192 * s) for s in SPC]
OFF3 = [56, 1 << 20, (2 << 20) + 8]
CL3 = [1024 * s for s in SPC]
PAD3 = [38, 42, 46]
# one segment; the whole object 1 (four); over a primary boundary (two); empty
RS4, ST4, LN4 = [0, 1, 2, 2], [100, 0, 9216 - 5, 7], [50, 1 << 30, 10, 0]
CO4 = [0, 64, 64 + 20448, 64 + 20448 + 16]
NSEG4 = 7


def _need(nreq=4, nseg=NSEG4):
    return _lib.lib().chipd_read_scratch_len(nreq, nseg)


def _read(in_off=OFF3, in_len=LEN3, rs=RS4, start=ST4, length=LN4, co=CO4, enc=STR, out=OUT, hashes=HASH, stat=STAT,
          used=USED, scratch=SCR, scratch_len=None, nreq=None, arrays=True, clen=True, chunk_len=CL3):
    nreq = len(rs) if nreq is None else nreq
    got = (ctypes.c_uint64 * 8)()
    scratch_len = _need() if scratch_len is None else scratch_len
    rc = _lib.lib().chipd_read_ranges_dev(enc, _u64(in_off), _u64(in_len) if arrays else None, hashes, _u32(PAD3),
                                          _u32(chunk_len), len(in_len), _u32(rs), _u64(start), _u64(length), nreq, out,
                                          _u64(co), got if clen else None, stat, used, scratch, scratch_len, None)
    return rc, list(got)[:4]


def test_read_argument_errors_need_no_device():
    import torch
    last = NO_DEVICE if not torch.cuda.is_available() else None

    def rc(**kw):
        return _read(**kw)[0]
    # NULL arrays or buffers with nreq > 0
    assert rc(arrays=False) == INVALID_ARG and rc(clen=False) == INVALID_ARG and rc(enc=None) == INVALID_ARG
    assert rc(out=None) == INVALID_ARG and rc(stat=None) == INVALID_ARG and rc(used=None) == INVALID_ARG
    assert rc(scratch=None) == INVALID_ARG
    assert rc(nreq=1 << 31) == INVALID_ARG
    # a request of a stream that is not there; a start or len above 2^53
    assert rc(rs=[0, 1, 3, 2]) == INVALID_ARG
    assert rc(start=[100, (1 << 53) + 1, 5, 7]) == INVALID_ARG and rc(length=[50, 1, (1 << 53) + 1, 0]) == INVALID_ARG
    # stream addresses want 8, content addresses and the scratch 16
    assert rc(in_off=[60, OFF3[1], OFF3[2]]) == INVALID_ARG and rc(in_off=[56, OFF3[1] + 4, OFF3[2]]) == INVALID_ARG
    assert rc(co=[0, 72, CO4[2], CO4[3]]) == INVALID_ARG and rc(out=OUT + 8) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    # two content ranges that overlap (either order); an empty range overlaps nothing
    assert rc(co=[0, 48, CO4[2], CO4[3]]) == INVALID_ARG and rc(co=[CO4[2], 64, 48 + 20448, CO4[3]]) == INVALID_ARG
    if last:
        assert rc(co=[0, 64, CO4[2], 0]) == last
    # a scratch one byte short
    assert rc(scratch_len=_need() - 1) == INVALID_ARG
    # no bao stream has that length
    gap = [LEN3[0], LEN3[1] + 8, LEN3[2]]
    assert rc(in_len=gap) == TRUNCATED and rc(in_len=[7, LEN3[1], LEN3[2]]) == TRUNCATED
    # INVALID_ARG before BAO_TRUNCATED before HASH_DECODE
    assert rc(in_len=gap, co=[0, 72, CO4[2], CO4[3]]) == INVALID_ARG
    assert rc(in_len=gap, scratch=SCR + 8) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    assert rc(hashes=None, scratch_len=_need() - 1) == INVALID_ARG
    # nothing to do
    assert rc(nreq=0) == OK
    assert rc(nreq=0, arrays=False, enc=None, out=None, hashes=None, scratch=None, stat=None, used=None, clen=False) == OK
    # a well-formed call gets as far as the device and no further; the lengths are written before that
    if last:
        code, got = _read()
        assert code == last and got == [50, 4 * CL3[1] - PAD3[1], 10, 0]
        # a chunk_len that does not fit is that request's status, not the call's: no content, fewer segments
        code, got = _read(chunk_len=[1024, 5120 + 1024, 9216], scratch_len=_need(4, 3))
        assert code == last and got == [50, 0, 10, 0]


def _layout(cl, pad, rs, start, length, align):
    nreq = len(rs)
    off, ln = (ctypes.c_uint64 * max(nreq, 1))(), (ctypes.c_uint64 * max(nreq, 1))()
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _lib.lib().chipd_read_layout(_u32(cl), _u32(pad), len(cl), _u32(rs), _u64(start), _u64(length), nreq, align, off,
                                      ln, ctypes.byref(total), ctypes.byref(nseg))
    return rc, list(off)[:nreq], list(ln)[:nreq], total.value, nseg.value


def test_read_layout_matches_plain_arithmetic():
    rng = random.Random(20)
    most = 0
    for rnd in range(40):
        nstreams = rng.randrange(1, 9)
        cl = [1024 * rng.choice([1, 2, 3, 5, 8, 9, 33, 4096]) for _ in range(nstreams)]
        pad = [rng.randrange(4096) for _ in range(nstreams)]
        cl[0], pad[0] = (cl[0] + 7, pad[0]) if rnd % 3 == 0 else (cl[0], pad[0])  # a misfit chunk_len
        if rnd % 5 == 0 and nstreams > 1:
            pad[1] = 4 * cl[1] + 1                                               # padding past the shards
        rs, start, length = [], [], []
        for s in range(nstreams):
            C, n_obj = cl[s], max(4 * cl[s] - pad[s], 1)
            for st, ln in ((0, 1), (n_obj - 1, 1), (n_obj - 1, 100), (n_obj, 5), (n_obj + 3000, 1), (rng.randrange(n_obj), 0),
                           (0, 1 << 53), (max(C - 5, 0), 10), (rng.randrange(n_obj), rng.randrange(1, 5000)),
                           (4 * C - rng.randrange(1, 40), 64)):
                rs.append(s); start.append(st); length.append(ln)
        align = 16 * rng.randrange(1, 20)
        rc, off, ln, total, nseg = _layout(cl, pad, rs, start, length, align)
        assert rc == OK
        cur = segs = 0
        for r, s in enumerate(rs):
            C = cl[s]
            fits = C % 1024 == 0 and pad[s] <= 4 * C
            n_obj = 4 * C - pad[s] if fits else 0
            end = min(n_obj, start[r] + length[r])
            want = end - start[r] if start[r] < n_obj and length[r] else 0
            assert (off[r], ln[r]) == (cur, want), (rnd, r)
            cur += -(-want // align) * align
            mine = (end - 1) // C - start[r] // C + 1 if want else 0
            segs, most = segs + mine, max(most, mine)
        assert (total, nseg) == (cur, segs)
    assert most == 4  # a range over all four primaries was among them
    # outputs may be NULL; align must be a multiple of 16; the other refusals
    L = _lib.lib().chipd_read_layout
    assert L(_u32([1024]), _u32([3]), 1, _u32([0]), _u64([5]), _u64([9]), 1, 16, None, None, None, None) == OK
    for align in (0, 8, 24):
        assert _layout([1024], [3], [0], [5], [9], align)[0] == INVALID_ARG
    assert _layout([1024], [3], [1], [5], [9], 16)[0] == INVALID_ARG
    assert _layout([1024], [3], [0], [(1 << 53) + 1], [9], 16)[0] == INVALID_ARG
    assert L(None, _u32([3]), 1, _u32([0]), _u64([5]), _u64([9]), 1, 16, None, None, None, None) == INVALID_ARG
    assert _layout([], [], [], [], [], 16) == (OK, [], [], 0, 0)
    # the scratch length: a multiple of 16, growing with requests and segments
    S = _lib.lib().chipd_read_scratch_len
    assert all(S(a, b) % 16 == 0 for a in (0, 1, 77) for b in (0, 1, 300))
    assert S(10, 10) <= S(11, 10) <= S(11, 40) and S(1000, 4000) > S(10, 40)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "read_plan_check.cpp")


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_read_plan_under_asan_ubsan(plan_check, seed):
    """Checks, layout, segments, slice requests and scratch layout of a ranged
    read are host code (read_plan.hpp): a stand-alone program drives them over
    seeded mixes (segments tile each request's object range exactly once, the
    window covers the columns, one slice request per segment and 8 status words,
    scratch regions disjoint inside the reported length) and multiplies
    the mask table's coefficients with the selected rows of the encoding matrix
    for all 163 masks of four or more shares."""
    assert "0 failures" in B.run_check(plan_check, seed)
