"""CPU tests of the fread boundary (include/carbonado_hip_fread.h): the chipf_*
symbols beside the nine older sets, their ctypes and Rust bindings, the errors
the calls decide before they touch a device, in the header's order, the layout
and scratch lengths, the bench tool's dry run, and the host plan and the text
the kernels compile (carbonado_amd/csrc/fread_plan.hpp, fread_device.hpp) as
stand-alone programs under ASan + UBSan."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import boundary as B
import test_read_cpu as RC
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_fread.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_fread.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"

OK, INVALID_ARG, HASH_DECODE, TRUNCATED, NO_DEVICE = 0, 1, 4, 6, 100
NAMES = {"chipf_abi_version", "chipf_index_scratch_len", "chipf_verify_index_dev", "chipf_frame_index_dev",
         "chipf_read_layout", "chipf_read_scratch_len", "chipf_read_ranges_dev"}
# the tenth boundary; boundary.BOUNDARIES holds the nine before it
MINE = B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7)


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipf_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports
    exported = B.exported()
    # assert_one_set's three comparisons, for a boundary that boundary.py does not list
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipf_abi_version() == 1
    assert "#define CHIPF_ABI_VERSION 1" in HEADER.read_text()
    # every older boundary keeps its count (62 / 5 / 6 / 4 / 4 / 3 / 10 / 10 / 8); no prefix clashes, no shared name
    assert [b.exports for b in B.BOUNDARIES] == [62, 5, 6, 4, 4, 3, 10, 10, 8]
    for b in B.BOUNDARIES:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the stream arguments are those of chipv_read_ranges_dev, in its order
    vread = RS._strip_comments((ROOT / "include" / "carbonado_hip_vread.h").read_text())
    vargs = re.search(r"chipv_read_ranges_dev\s*\(([^)]*)\)", vread, flags=re.S).group(1)
    vnames = [re.match(r".*?(\w+)$", p.strip()).group(1) for p in " ".join(vargs.split()).split(",")]
    streams = vnames[:vnames.index("nstreams") + 1]
    head = ["format", "keys", "ivs", "key_status"]
    assert [n for n, _ in protos["chipf_verify_index_dev"][1]] == head + streams + [
        "frame_off", "idx_off", "nframes", "d_index_status", "d_plain_len", "d_index_vouch", "d_scratch", "scratch_len",
        "stream"]
    assert [n for n, _ in protos["chipf_frame_index_dev"][1]] == head + streams + [
        "frame_off", "idx_off", "idx_cap", "nframes", "index_status", "plain_len", "index_vouch", "d_scratch",
        "scratch_len", "stream"]
    assert [n for n, _ in protos["chipf_read_ranges_dev"][1]] == [
        "format", "keys", "ivs", "index_status", "frame_off", "idx_off", "nframes", "plain_len"] + vnames
    assert [n for n, _ in protos["chipf_read_scratch_len"][1]] == ["nreq", "nseg", "stage_total", "vseg", "nstreams"]


def test_ffi_fread_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipf_"), prototypes())
    assert re.search(r"pub const CHIPF_ABI_VERSION: c_int = 1;", B.ffi_text(FFI))


WRAPPERS = (("frame_index_scratch", ("chipf_index_scratch_len",)), ("frame_index", ("chipf_frame_index_dev",)),
            ("verify_frame_index", ("chipf_verify_index_dev",)), ("frame_read_layout", ("chipf_read_layout",)),
            ("frame_read_scratch", ("chipf_read_scratch_len",)), ("read_frame_ranges", ("chipf_read_ranges_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_fread;", lib, flags=re.M) and "chipf_abi_version" in lib
    for fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {fn}\(", lib)
        assert m, fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {fn}\(", src, flags=re.M), fn
        for call in calls:
            assert f"ffi_fread::{call}(" in body, (fn, call)
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
STR, OUT, HASH, STAT, USED, SCR = RC.STR, RC.OUT, RC.HASH, RC.STAT, RC.USED, RC.SCR
VOUCH, PLAIN = 0x77000000, 0x79000000
# test_read_cpu's three streams as level-14 streams: L = 4 C - padding
L14 = [4 * c - p for c, p in zip(RC.CL3, RC.PAD3)]
INDEX = [[10, L14[0]], [10, 9000, L14[1]], [10, L14[2]]]
IDX_OFF, NFRAMES, PLAIN_LEN = [0, 2, 5], [1, 2, 1], [100, 65536 + 5, 65536]
FRAME_OFF = [x for i in INDEX for x in i]


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def _layout(rs, start, length, fmt=14, frame_off=FRAME_OFF, nframes=NFRAMES, plain=PLAIN_LEN, align=16, istat=None):
    u64, u32 = RC._u64, RC._u32
    nreq = len(rs)
    off, ln = (ctypes.c_uint64 * max(nreq, 1))(), (ctypes.c_uint64 * max(nreq, 1))()
    out = [ctypes.c_uint64() for _ in range(4)]
    rc = _lib.lib().chipf_read_layout(fmt, u32(RC.CL3), u32(RC.PAD3), u32(istat) if istat else None, u64(frame_off),
                                      u64(IDX_OFF), u64(nframes), u64(plain), 3, u32(rs), u64(start), u64(length), nreq,
                                      align, off, ln, *(ctypes.byref(o) for o in out))
    return rc, list(off)[:nreq], list(ln)[:nreq], [o.value for o in out]


RS6, ST6, LN6 = [0, 1, 1, 2, 1, 0], [0, 65530, 100, 65535, 65541, 7], [1 << 30, 100, 50, 10, 5, 0]


def test_read_layout_counts_frames_rows_and_segments():
    rc, off, ln, (total, nseg, stage, vseg) = _layout(RS6, ST6, LN6)
    assert rc == OK and ln == [100, 11, 50, 1, 0, 0] and off == [0, 112, 128, 192, 208, 208] and total == 208
    assert nseg == 1 + 2 + 1 + 1
    up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    rows = [L14[0] - 10, L14[1] - 10, 9000 - 10, L14[2] - 10]
    assert stage == sum(up16(r) for r in rows)
    # the vouched read's segments: the rows as object ranges through chipd_read_layout
    want = RC._layout(RC.CL3, RC.PAD3, [0, 1, 1, 2], [10] * 4, rows, 16)
    assert vseg == want[4]
    assert _layout(RS6, ST6, LN6, align=64)[1] == [0, 128, 192, 256, 320, 320]
    # a killed stream's requests claim their range and count nothing else; its index is not looked at
    rc, off, ln, (total, nseg, stage, vseg) = _layout(RS6, ST6, LN6, istat=[0, 16, 0],
                                                      frame_off=[10, L14[0], 0, 0, 0, 10, L14[2]])
    assert rc == OK and ln == [100, 11, 50, 1, 0, 0] and nseg == 2 and stage == up16(rows[0]) + up16(rows[3])
    for bad in (dict(fmt=13), dict(fmt=12), dict(align=0), dict(align=8), dict(frame_off=[10, L14[0], 10, 10, L14[1], 10, L14[2]]),
                dict(frame_off=[10, L14[0], 10, 9000, L14[1] - 1, 10, L14[2]]), dict(plain=[100, 65536, 65536]),
                dict(plain=[100, 65536 + 5, 65537]), dict(nframes=[1, 1, 1]), dict(fmt=15)):
        assert _layout(RS6, ST6, LN6, **bad)[0] == INVALID_ARG, bad
    assert _layout([3], [0], [5])[0] == INVALID_ARG and _layout([0], [(1 << 53) + 1], [5])[0] == INVALID_ARG
    L = _lib.lib()
    assert L.chipf_read_layout(14, None, None, None, None, None, None, None, 3, None, None, None, 1, 16, None, None, None,
                               None, None, None) == INVALID_ARG
    assert L.chipf_read_layout(14, None, None, None, None, None, None, None, 0, None, None, None, 0, 16, None, None, None,
                               None, None, None) == OK


def test_scratch_lengths_are_multiples_of_16_and_grow():
    L = _lib.lib()
    for ns, ne in ((1, 1), (3, 7), (1024, 17408)):
        s = L.chipf_index_scratch_len(ns, ne)
        assert s % 16 == 0 and s >= 16 * ne + 8 * ne + L.chipv_read_scratch_len(ne, ne) + L.chipc_ctr_scratch_len(ns, ne)
        assert L.chipf_index_scratch_len(ns + 1, ne) > s and L.chipf_index_scratch_len(ns, ne + 2) > s
    assert L.chipf_index_scratch_len(1 << 31, 1) == 0 and L.chipf_index_scratch_len(1, 1 << 30) == 0
    for nreq, nseg, stage, vseg, ns in ((1, 1, 16, 1, 1), (6, 5, 70000, 8, 3), (16384, 17354, 1 << 30, 19671, 1024)):
        s = L.chipf_read_scratch_len(nreq, nseg, stage, vseg, ns)
        assert s % 16 == 0 and s >= stage + L.chipv_read_scratch_len(nreq, vseg) + L.chipc_ctr_scratch_len(ns, nreq)
        assert L.chipf_read_scratch_len(nreq + 1, nseg, stage, vseg, ns) > s
        assert L.chipf_read_scratch_len(nreq, nseg + 4, stage, vseg, ns) > s
        assert L.chipf_read_scratch_len(nreq, nseg, stage + 16, vseg, ns) > s
        assert L.chipf_read_scratch_len(nreq, nseg, stage, vseg + 64, ns) > s
        assert L.chipf_read_scratch_len(nreq, nseg, stage, vseg, ns + 1) > s
    assert L.chipf_read_scratch_len(1 << 31, 1, 16, 1, 1) == 0


def test_index_calls_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    kk, vv = (ctypes.c_uint8 * 96)(), (ctypes.c_uint8 * 48)()
    need = L.chipf_index_scratch_len(3, 7)
    host = dict(fo=(ctypes.c_uint64 * 16)(), nf=(ctypes.c_uint64 * 3)(), st=(ctypes.c_uint32 * 3)(),
                pl=(ctypes.c_uint64 * 3)(), vo=(ctypes.c_uint32 * 3)())

    def verify(fmt=14, keys=kk, ivs=vv, in_off=RC.OFF3, in_len=RC.LEN3, enc=STR, hashes=HASH, fo=FRAME_OFF, nf=NFRAMES,
               stat=STAT, plain=PLAIN, vouch=VOUCH, scratch=SCR, scratch_len=need, ns=3, arrays=True):
        return L.chipf_verify_index_dev(fmt, keys, ivs, None, enc, u64(in_off), u64(in_len) if arrays else None, hashes,
                                        u32(RC.PAD3), u32(RC.CL3), ns, u64(fo), u64(IDX_OFF), u64(nf), stat, plain, vouch,
                                        scratch, scratch_len, None)

    def build(fmt=14, keys=kk, ivs=vv, in_off=RC.OFF3, in_len=RC.LEN3, enc=STR, hashes=HASH, cap=(2, 3, 2), out=True,
              scratch=SCR, scratch_len=need, ns=3, arrays=True):
        return L.chipf_frame_index_dev(fmt, keys, ivs, None, enc, u64(in_off), u64(in_len) if arrays else None, hashes,
                                       u32(RC.PAD3), u32(RC.CL3), ns, host["fo"], u64(IDX_OFF), u64(list(cap)),
                                       host["nf"] if out else None, host["st"], host["pl"], host["vo"], scratch,
                                       scratch_len, None)

    gap = [RC.LEN3[0], RC.LEN3[1] + 8, RC.LEN3[2]]
    for call in (verify, build):
        assert call(ns=0) == OK and call(ns=0, fmt=3, arrays=False, enc=None, scratch=None) == OK
        for fmt in (0, 12, 13, 16):
            assert call(fmt=fmt) == INVALID_ARG
        assert call(fmt=15, keys=None) == INVALID_ARG and call(fmt=15, ivs=None) == INVALID_ARG
        assert call(arrays=False) == INVALID_ARG and call(enc=None) == INVALID_ARG and call(scratch=None) == INVALID_ARG
        assert call(ns=1 << 31) == INVALID_ARG
        assert call(in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG and call(scratch=SCR + 8) == INVALID_ARG
        assert call(scratch_len=need - 1) == INVALID_ARG
        assert call(in_len=gap) == TRUNCATED and call(in_len=gap, scratch_len=need - 1) == INVALID_ARG
        assert call(in_len=gap, fmt=13) == INVALID_ARG and call(in_len=gap, scratch=SCR + 8) == INVALID_ARG
        assert call(hashes=None) == HASH_DECODE and call(hashes=None, in_len=gap) == TRUNCATED
        if last:
            assert call() == last and call(fmt=15) == last and call(keys=None, ivs=None) == last
    assert verify(stat=None) == INVALID_ARG and verify(plain=None) == INVALID_ARG and verify(vouch=None) == INVALID_ARG
    assert verify(nf=[1, 1 << 30, 1], scratch_len=1 << 60) == INVALID_ARG
    assert verify(fo=[10, L14[0], 10, (1 << 53) + 1, L14[1], 10, L14[2]]) == INVALID_ARG
    assert build(out=False) == INVALID_ARG and build(cap=(2, 1 << 30, 2), scratch_len=1 << 60) == INVALID_ARG
    assert build(cap=(2, 4, 2)) == INVALID_ARG          # one entry more than the scratch was sized for
    if last:  # an index that is wrong is the device's to refuse, not the host's
        assert verify(fo=[L14[0], 10, 9000, 10, L14[1], 3, 4]) == last


def _read_numbers():
    return _layout(RS6, ST6, LN6)[3]


def test_read_argument_errors_in_their_order():
    u64, u32 = RC._u64, RC._u32
    L = _lib.lib()
    last = _last()
    kk, vv = (ctypes.c_uint8 * 96)(), (ctypes.c_uint8 * 48)()
    _, nseg, stage, vseg = _read_numbers()
    need = L.chipf_read_scratch_len(6, nseg, stage, vseg, 3)
    CO6 = [3, 120, 140, 200, 250, 250]

    def call(fmt=14, keys=kk, ivs=vv, istat=None, fo=FRAME_OFF, nf=NFRAMES, plain=PLAIN_LEN, in_off=RC.OFF3,
             in_len=RC.LEN3, rs=RS6, start=ST6, length=LN6, co=CO6, enc=STR, out=OUT, hashes=HASH, stat=STAT, used=USED,
             vouch=VOUCH, flags=0, scratch=SCR, scratch_len=need, nreq=None, arrays=True, clen=True, index=True):
        got = (ctypes.c_uint64 * 8)()
        rc = L.chipf_read_ranges_dev(fmt, keys, ivs, u32(istat) if istat else None, u64(fo) if index else None,
                                     u64(IDX_OFF), u64(nf), u64(plain), enc, u64(in_off), u64(in_len) if arrays else None,
                                     hashes, u32(RC.PAD3), u32(RC.CL3), 3, u32(rs), u64(start), u64(length),
                                     len(rs) if nreq is None else nreq, out, u64(co), got if clen else None, stat, used,
                                     vouch, flags, scratch, scratch_len, None)
        return rc, list(got)[:6]

    def rc(**kw):
        return call(**kw)[0]

    assert rc(nreq=0) == OK and rc(nreq=0, fmt=3, index=False, arrays=False, enc=None, out=None, scratch=None) == OK
    assert rc(fmt=15, keys=None) == INVALID_ARG and rc(fmt=15, ivs=None) == INVALID_ARG and rc(index=False) == INVALID_ARG
    assert rc(arrays=False) == INVALID_ARG and rc(clen=False) == INVALID_ARG and rc(enc=None) == INVALID_ARG
    assert rc(stat=None) == INVALID_ARG and rc(used=None) == INVALID_ARG and rc(vouch=None) == INVALID_ARG
    assert rc(scratch=None) == INVALID_ARG
    for fmt in (0, 12, 13, 16):
        assert rc(fmt=fmt) == INVALID_ARG
    for f in (2, 4, 3, 1 << 31):
        assert rc(flags=f) == INVALID_ARG
    assert rc(nreq=1 << 31) == INVALID_ARG
    assert rc(rs=[0, 1, 3, 2, 1, 0]) == INVALID_ARG
    assert rc(start=[0, (1 << 53) + 1, 100, 65535, 65541, 7]) == INVALID_ARG
    assert rc(length=[1 << 30, 100, (1 << 53) + 1, 10, 5, 0]) == INVALID_ARG
    assert rc(fo=[10, L14[0], 10, 10, L14[1], 10, L14[2]]) == INVALID_ARG            # entries that do not ascend
    assert rc(fo=[10, L14[0], 10, 9000, L14[1] + 1, 10, L14[2]]) == INVALID_ARG      # a last entry that is not L
    assert rc(plain=[100, 65536, 65536]) == INVALID_ARG and rc(fmt=15) == INVALID_ARG
    assert rc(out=None) == INVALID_ARG
    assert rc(in_off=[60, RC.OFF3[1], RC.OFF3[2]]) == INVALID_ARG and rc(scratch=SCR + 8) == INVALID_ARG
    assert rc(co=[3, 100, 140, 200, 250, 250]) == INVALID_ARG                        # content ranges that overlap
    assert rc(scratch_len=need - 1) == INVALID_ARG
    gap = [RC.LEN3[0], RC.LEN3[1] + 8, RC.LEN3[2]]
    assert rc(in_len=gap) == TRUNCATED and rc(in_len=gap, scratch_len=need - 1) == INVALID_ARG
    assert rc(in_len=gap, co=[3, 100, 140, 200, 250, 250]) == INVALID_ARG and rc(in_len=gap, flags=2) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE and rc(hashes=None, in_len=gap) == TRUNCATED
    if last:
        for f in (0, 1):
            code, got = call(flags=f)
            assert code == last and got == [100, 11, 50, 1, 0, 0]
        # content at any byte offset; a killed stream's index is not looked at and its requests still claim their ranges
        code, got = call(istat=[0, 11, 0], fo=[10, L14[0], 0, 0, 0, 10, L14[2]])
        assert code == last and got == [100, 11, 50, 1, 0, 0]
        assert rc(istat=[0, 11, 0], co=[3, 100, 140, 200, 250, 250]) == INVALID_ARG
        assert rc(keys=None, ivs=None) == last


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "fread_plan_check.cpp", include=[CSRC])


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_fread_plan_under_asan_ubsan(plan_check, seed):
    """Request -> frames -> staging rows -> work items against a brute-force
    per-byte map over seeded indexes, the index check's header reads, the
    scratch lengths and the order of the errors."""
    out = B.run_check(plan_check, seed, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


@pytest.fixture(scope="module")
def device_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "fread_device_check.cpp", include=[CSRC],
                         extra_sources=[CSRC / "host_snap.cpp"])


def test_fread_device_text_under_asan_ubsan(device_check):
    """The text the kernels compile, on one host thread:
    the walk and the chain check over streams written by the host's
    compressor and over hand-built ones, wrong indexes, and a frame served as
    the block kernel serves it at every start and end residue mod 16."""
    out = B.run_check(device_check, timeout=600)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_fread_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fread_bench.py"), "--dry"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "fread_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["object_bytes"] == 1 << 20 and res["range_bytes"] == 4096
    assert res["frames_per_stream"] == 16 and res["index_scratch_bytes"] > 0
    assert res["read_1"]["requests"] == 1024 and res["read_16"]["requests"] == 16384
    assert 1024 <= res["read_1"]["work_items"] <= 2048
    assert res["read_16"]["scratch_bytes"] > res["read_16"]["staging_bytes"] > 16 * 1024 * 65536
    assert res["launches"]["vouched_read"] == 8 and res["launches"]["keystream"] == 2
