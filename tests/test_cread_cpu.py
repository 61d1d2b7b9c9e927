"""CPU tests of the cread boundary (include/carbonado_hip_cread.h): the chipc_*
symbols beside the eight older sets, their ctypes and Rust bindings, every
error the three calls decide before they touch a device, in the header's order,
the scratch and layout lengths, the bench tool's dry run, and the keystream
arithmetic and the host plan (carbonado_amd/csrc/cread_device.hpp,
cread_plan.hpp) as a stand-alone program under ASan + UBSan against EVP
AES-256-GCM."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import test_read_cpu as RC
import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_cread.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_cread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, ECIES, NO_DEVICE = 0, 1, 4, 6, 17, 100
NAMES = {"chipc_abi_version", "chipc_ctr_scratch_len", "chipc_ctr_ranges_dev", "chipc_stream_keys_scratch_len",
         "chipc_stream_keys_dev", "chipc_read_layout", "chipc_read_scratch_len", "chipc_read_ranges_dev"}


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipc_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == 8
    exported = B.exported()
    B.assert_one_set(protos, exported, "chipc_")
    assert _lib.lib().chipc_abi_version() == 1
    assert "#define CHIPC_ABI_VERSION 1" in HEADER.read_text()
    # the eight older boundaries keep their sets; "chipc_" is a prefix of none of theirs and none is a prefix of it
    B.assert_older_keep_their_sets(exported, "chipc_")
    # the argument lists the issue fixes
    assert [n for n, _ in protos["chipc_ctr_ranges_dev"][1]] == [
        "keys", "ivs", "nkeys", "item_key", "pos", "n", "nitems", "d_buf", "buf_off", "d_gate", "d_scratch",
        "scratch_len", "stream"]
    assert [n for n, _ in protos["chipc_stream_keys_dev"][1]] == [
        "secret_key", "sk_len", "d_streams", "in_off", "in_len", "d_hash", "padding", "chunk_len", "nstreams",
        "keys_out", "ivs_out", "key_status", "d_scratch", "scratch_len", "stream"]
    assert [n for n, _ in protos["chipc_read_layout"][1]] == [
        "chunk_len", "padding", "nstreams", "req_stream", "start", "len", "nreq", "align", "content_off", "content_len",
        "content_total", "nseg"]
    vread = RS._strip_comments((ROOT / "include" / "carbonado_hip_vread.h").read_text())
    vargs = re.search(r"chipv_read_ranges_dev\s*\(([^)]*)\)", vread, flags=re.S).group(1)
    vnames = [re.match(r".*?(\w+)$", p.strip()).group(1) for p in " ".join(vargs.split()).split(",")]
    assert [n for n, _ in protos["chipc_read_ranges_dev"][1]] == ["keys", "ivs", "key_status"] + vnames
    assert [n for n, _ in protos["chipc_read_scratch_len"][1]] == ["nreq", "nseg", "nstreams"]


def test_ffi_cread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipc_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPC_ABI_VERSION: c_int = 1;", text)


WRAPPERS = (("ctr_scratch", ("chipc_ctr_scratch_len",)), ("ctr_ranges", ("chipc_ctr_ranges_dev",)),
            ("stream_keys_scratch", ("chipc_stream_keys_scratch_len",)), ("stream_keys", ("chipc_stream_keys_dev",)),
            ("plain_read_layout", ("chipc_read_layout",)), ("plain_read_scratch", ("chipc_read_scratch_len",)),
            ("read_plain_ranges", ("chipc_read_ranges_dev",)))


def test_lib_rs_has_the_safe_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    assert re.search(r"^mod ffi_cread;", lib, flags=re.M)
    for fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        for call in calls:
            assert f"ffi_cread::{call}(" in body, (fn, call)
    assert "chipc_abi_version" in lib


def test_device_module_has_the_bindings():
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    for fn, calls in WRAPPERS:
        assert re.search(rf"^def {fn}\(", src, flags=re.M), fn
        for call in calls:
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
BUF, GATE, SCR = 0x10000000, 0x74000000, 0x78000000
STR, OUT, HASH, STAT, USED, VOUCH = RC.STR, RC.OUT, RC.HASH, RC.STAT, RC.USED, 0x77000000


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def test_ctr_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    keys, ivs = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 32)()
    IK, POS, N, OFF = [0, 1, 0, 1], [5, 0, 99, 1 << 30], [100, 0, 17, 5000], [0, 8, 112, 144]
    need = L.chipc_ctr_scratch_len(2, 4)

    def rc(keys=keys, ivs=ivs, nkeys=2, ik=IK, pos=POS, n=N, nitems=None, buf=BUF, off=OFF, scratch=SCR,
           scratch_len=need, arrays=True):
        a64 = (lambda x: u64(x)) if arrays else (lambda x: None)
        return L.chipc_ctr_ranges_dev(keys, ivs, nkeys, u32(ik) if arrays else None, a64(pos), a64(n),
                                      len(n) if nitems is None else nitems, buf, a64(off), GATE, scratch, scratch_len,
                                      None)

    assert rc(nitems=0) == OK and rc(nitems=0, keys=None, ivs=None, arrays=False, buf=None, scratch=None) == OK
    assert rc(keys=None) == INVALID_ARG and rc(ivs=None) == INVALID_ARG and rc(arrays=False) == INVALID_ARG
    assert rc(scratch=None) == INVALID_ARG
    assert rc(nitems=1 << 31) == INVALID_ARG
    assert rc(ik=[0, 2, 0, 1]) == INVALID_ARG and rc(nkeys=1) == INVALID_ARG
    assert rc(pos=[5, 0, 99, (1 << 36) - 32 - 4999]) == INVALID_ARG and rc(pos=[5, 0, (1 << 64) - 1, 3]) == INVALID_ARG
    assert rc(n=[100, (1 << 36) - 31, 17, 5000], scratch_len=1 << 60) == INVALID_ARG
    assert rc(off=[0, 8, 112, (1 << 53) + 16]) == INVALID_ARG
    assert rc(buf=None) == INVALID_ARG
    assert rc(off=[0, 8, 120, 144]) == INVALID_ARG and rc(buf=BUF + 4) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    assert rc(off=[0, 8, 96, 144]) == INVALID_ARG and rc(off=[0, 8, 112, 128]) == INVALID_ARG
    assert rc(scratch_len=need - 1) == INVALID_ARG
    # precedence: the key index before the position, the alignment before the overlap, both before the scratch length
    assert rc(ik=[0, 2, 0, 1], pos=[5, 0, 99, 1 << 40]) == INVALID_ARG
    assert rc(off=[0, 8, 104, 144], scratch_len=0) == INVALID_ARG
    if last:
        assert rc() == last
        assert rc(pos=[5, 0, 99, (1 << 36) - 32 - 5000]) == last        # ends exactly at the limit
        assert rc(off=[0, 3, 112, 144]) == last                         # (an empty item's offset is not looked at)
        assert rc(n=[0, 0, 0, 0], buf=None, off=[1, 2, 3, 4]) == last
        assert rc(off=[0, 8, 112, 129 + 15]) == last and rc(off=[5008, 8, 5120, 0]) == last


def _layout(fn, rs, start, length, cl=RC.CL3, pad=RC.PAD3, align=16):
    u64, u32 = RC._u64, RC._u32
    nreq = len(rs)
    off, ln = (ctypes.c_uint64 * max(nreq, 1))(), (ctypes.c_uint64 * max(nreq, 1))()
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    rc = fn(u32(cl), u32(pad), len(cl), u32(rs), u64(start), u64(length), nreq, align, off, ln, ctypes.byref(total),
            ctypes.byref(nseg))
    return rc, list(off)[:nreq], list(ln)[:nreq], total.value, nseg.value


# plaintext requests over test_read_cpu's three streams (P = 4 C - padding - 97: 3961, 20341, 36721)
P3 = [4 * c - p - 97 for c, p in zip(RC.CL3, RC.PAD3)]
RS5, ST5, LN5 = [0, 1, 2, 2, 1], [100, 0, 9216 - 97 - 5, 7, 20000], [50, 1 << 30, 10, 0, 4096]


def test_read_layout_is_the_envelope_layout_shifted():
    L = _lib.lib()
    cases = [(RS5, ST5, LN5, RC.CL3, RC.PAD3),
             ([0, 0, 0, 0], [P3[0], P3[0] + 1, P3[0] - 1, P3[0] - 10], [5, 5, 5, 100], RC.CL3, RC.PAD3),  # start >= P, clipped
             ([0, 0, 1], [0, 5, 0], [10, 1, 1 << 20], [1024, 5120, 9216], [4096 - 50, 42, 46]),         # P < 0: no content
             ([0, 1], [0, 0], [10, 7], [1024, 5120, 9216], [4096 - 97, 4 * 5120 - 98, 46]),              # P = 0 and P = 1
             ([2, 1, 0], [36720, 1023 - 97, 4 * 1024 - 38 - 97 - 1], [1, 2, 1], RC.CL3, RC.PAD3)]
    for rs, start, length, cl, pad in cases:
        got = _layout(L.chipc_read_layout, rs, start, length, cl, pad)
        want = _layout(L.chipd_read_layout, rs, [s + 97 for s in start], length, cl, pad)
        assert got[0] == OK and got == want, (rs, start)
        plain = [max(4 * cl[s] - pad[s] - 97, 0) for s in rs]
        assert got[2] == [max(min(p, a + n) - a, 0) for p, a, n in zip(plain, start, length)]
    assert _layout(L.chipc_read_layout, [0], [0], [5], align=8)[0] == INVALID_ARG
    assert _layout(L.chipc_read_layout, [3], [0], [5])[0] == INVALID_ARG
    assert _layout(L.chipc_read_layout, [0], [(1 << 53) - 96], [5])[0] == INVALID_ARG
    assert _layout(L.chipc_read_layout, [0], [(1 << 64) - 1], [5])[0] == INVALID_ARG
    assert L.chipc_read_layout(None, None, 3, None, None, None, 1, 16, None, None, None, None) == INVALID_ARG
    assert L.chipc_read_layout(None, None, 0, None, None, None, 0, 16, None, None, None, None) == OK


def test_scratch_lengths_are_multiples_of_16_and_grow():
    L = _lib.lib()
    for nkeys, nitems in ((0, 1), (1, 1), (3, 150), (1024, 1024), (5, 100000)):
        s = L.chipc_ctr_scratch_len(nkeys, nitems)
        assert s % 16 == 0 and s >= 40 * nitems + (48 + 512) * nkeys
        assert L.chipc_ctr_scratch_len(nkeys + 1, nitems) > s and L.chipc_ctr_scratch_len(nkeys, nitems + 1) >= s
        assert L.chipc_ctr_scratch_len(nkeys, nitems + 2) > s
    assert L.chipc_ctr_scratch_len(1, 1 << 31) == 0
    for ns in (1, 2, 8, 1024):
        s = L.chipc_stream_keys_scratch_len(ns)
        assert s % 16 == 0 and s >= 96 * ns + 12 * ns + L.chipv_read_scratch_len(ns, ns)
        assert L.chipc_stream_keys_scratch_len(ns + 1) > s
    for nreq, nseg, ns in ((1, 1, 1), (5, 8, 3), (1024, 1024, 1024), (250, 300, 8)):
        s = L.chipc_read_scratch_len(nreq, nseg, ns)
        assert s % 16 == 0 and s >= L.chipv_read_scratch_len(nreq, nseg) + L.chipc_ctr_scratch_len(ns, nreq)
        assert L.chipc_read_scratch_len(nreq + 16, nseg, ns) > s and L.chipc_read_scratch_len(nreq, nseg + 64, ns) > s
        assert L.chipc_read_scratch_len(nreq, nseg, ns + 1) > s


def _keys_need(ns=3):
    return _lib.lib().chipc_stream_keys_scratch_len(ns)


def test_stream_keys_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    secret = bytes(range(1, 33))
    keys, ivs, stat = (ctypes.c_uint8 * 96)(), (ctypes.c_uint8 * 48)(), (ctypes.c_uint32 * 3)()

    def rc(sk=secret, in_off=RC.OFF3, in_len=RC.LEN3, enc=STR, hashes=HASH, keys=keys, ivs=ivs, stat=stat, scratch=SCR,
           scratch_len=None, ns=3, arrays=True, cl=RC.CL3):
        scratch_len = _keys_need() if scratch_len is None else scratch_len
        return L.chipc_stream_keys_dev(sk, len(sk) if sk else 0, enc, u64(in_off), u64(in_len) if arrays else None,
                                       hashes, u32(RC.PAD3), u32(cl), ns, keys, ivs, stat, scratch, scratch_len, None)

    assert rc(ns=0) == OK
    assert rc(sk=None) == INVALID_ARG and rc(keys=None) == INVALID_ARG and rc(ivs=None) == INVALID_ARG
    assert rc(stat=None) == INVALID_ARG and rc(scratch=None) == INVALID_ARG and rc(arrays=False) == INVALID_ARG
    assert rc(enc=None) == INVALID_ARG
    assert rc(in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG           # what the vouched read refuses
    assert rc(scratch=SCR + 8) == INVALID_ARG and rc(scratch_len=_keys_need() - 1) == INVALID_ARG
    gap = [RC.LEN3[0], RC.LEN3[1] + 8, RC.LEN3[2]]
    assert rc(in_len=gap) == TRUNCATED and rc(in_len=gap, scratch=SCR + 8) == INVALID_ARG
    assert rc(in_len=gap, scratch_len=_keys_need() - 1) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    assert rc(sk=bytes(32)) == ECIES and rc(sk=secret[:31]) == ECIES and rc(sk=b"\xff" * 32) == ECIES
    assert rc(sk=bytes(32), hashes=None) == HASH_DECODE and rc(sk=bytes(32), in_len=gap) == TRUNCATED
    assert rc(sk=bytes(32), scratch=SCR + 8) == INVALID_ARG
    if last:
        assert rc() == last


def _read_need(nreq=5, nseg=None, ns=3):
    L = _lib.lib()
    if nseg is None:
        nseg = _layout(L.chipc_read_layout, RS5, ST5, LN5)[4]
    return L.chipc_read_scratch_len(nreq, nseg, ns)


def test_read_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    kk, vv = (ctypes.c_uint8 * 96)(), (ctypes.c_uint8 * 48)()
    _, CO5, CL5, _, nseg = _layout(L.chipc_read_layout, RS5, ST5, LN5)
    assert CL5 == [50, P3[1], 10, 0, 341] and nseg == 1 + 4 + 2 + 0 + 1

    def call(keys=kk, ivs=vv, kstat=None, in_off=RC.OFF3, in_len=RC.LEN3, rs=RS5, start=ST5, length=LN5, co=CO5, enc=STR,
             out=OUT, hashes=HASH, stat=STAT, used=USED, vouch=VOUCH, flags=0, scratch=SCR, scratch_len=None, nreq=None,
             arrays=True, clen=True, cl=RC.CL3):
        got = (ctypes.c_uint64 * 8)()
        scratch_len = _read_need() if scratch_len is None else scratch_len
        rc = L.chipc_read_ranges_dev(keys, ivs, u32(kstat) if kstat else None, enc, u64(in_off),
                                     u64(in_len) if arrays else None, hashes, u32(RC.PAD3), u32(cl), len(in_len), u32(rs),
                                     u64(start), u64(length), len(rs) if nreq is None else nreq, out, u64(co),
                                     got if clen else None, stat, used, vouch, flags, scratch, scratch_len, None)
        return rc, list(got)[:5]

    def rc(**kw):
        return call(**kw)[0]

    assert rc(nreq=0) == OK and rc(nreq=0, keys=None, ivs=None, arrays=False, enc=None, out=None, scratch=None) == OK
    assert rc(keys=None) == INVALID_ARG and rc(ivs=None) == INVALID_ARG
    # the vouched read's list, in its order
    assert rc(arrays=False) == INVALID_ARG and rc(clen=False) == INVALID_ARG and rc(enc=None) == INVALID_ARG
    assert rc(out=None) == INVALID_ARG and rc(stat=None) == INVALID_ARG and rc(used=None) == INVALID_ARG
    assert rc(vouch=None) == INVALID_ARG and rc(scratch=None) == INVALID_ARG
    for f in (2, 4, 3, 1 << 31):
        assert rc(flags=f) == INVALID_ARG
    assert rc(nreq=1 << 31) == INVALID_ARG
    assert rc(rs=[0, 1, 3, 2, 1]) == INVALID_ARG
    assert rc(start=[100, (1 << 53) - 96, 5, 7, 0]) == INVALID_ARG and rc(length=[50, 1, (1 << 53) + 1, 0, 1]) == INVALID_ARG
    assert rc(in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG
    assert rc(co=[0, 72, CO5[2], CO5[3], CO5[4]]) == INVALID_ARG and rc(out=OUT + 8) == INVALID_ARG
    assert rc(scratch=SCR + 8) == INVALID_ARG
    assert rc(co=[0, 48, CO5[2], CO5[3], CO5[4]]) == INVALID_ARG
    assert rc(scratch_len=_read_need() - 1) == INVALID_ARG
    assert rc(scratch_len=L.chipv_read_scratch_len(5, nseg)) == INVALID_ARG    # the vouched read's own is too short
    gap = [RC.LEN3[0], RC.LEN3[1] + 8, RC.LEN3[2]]
    assert rc(in_len=gap) == TRUNCATED
    assert rc(in_len=gap, co=[0, 72, CO5[2], CO5[3], CO5[4]]) == INVALID_ARG
    assert rc(in_len=gap, flags=2) == INVALID_ARG and rc(in_len=gap, keys=None) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    assert rc(hashes=None, scratch_len=_read_need() - 1) == INVALID_ARG
    if last:
        for f in (0, 1):
            code, got = call(flags=f)
            assert code == last and got == CL5
        # the content lengths are the layout's whatever the key status; a killed request still claims its range
        code, got = call(kstat=[0, 17, 7])
        assert code == last and got == CL5
        assert rc(kstat=[0, 17, 7], co=[0, 48, CO5[2], CO5[3], CO5[4]]) == INVALID_ARG


@pytest.fixture(scope="module")
def cread_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "cread_device_check.cpp", libs=["crypto"])


def test_cread_device_and_plan_under_asan_ubsan(cread_check):
    """The text the kernels compile, on the host, against EVP AES-256-GCM:
    items walked lane by lane as KC splits them, the neighbour exchange
    modelled (lane 63 is handed poison), every pos % 16 times the length edges
    and the span edges, positions around 8192, the lite key setup's J0 against
    its definition, the committed counter-wrap pair, killed items and the plan's
    checks."""
    out = B.run_check(cread_check, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_cread_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "cread_bench.py"), "--dry"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "cread_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["object_bytes"] == (1 << 20) - 41 - 97 and res["range_bytes"] == 4096
    assert res["requests"] == 1024 and res["damaged_streams"] == 16
    assert res["read_scratch_bytes"] > res["vread_scratch_bytes"] > 0 and res["keys_scratch_bytes"] > 0
    assert res["launches"] == {"vouched_read": 8, "keystream": 2}
