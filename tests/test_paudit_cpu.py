"""CPU tests of the paudit boundary (include/carbonado_hip_paudit.h): the chipp_*
symbols beside the thirteen older sets, their ctypes and Rust bindings, the
errors the calls decide before they touch a device, in the header's order, the
table, scratch and proof-bound lengths, the bench tool's dry run, and the
planning text the plan kernel compiles (carbonado_amd/csrc/paudit_device.hpp)
with the host's O(1) share (paudit_plan.hpp) as a stand-alone program under
ASan + UBSan."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import boundary as B
import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "carbonado_hip_paudit.h"
FFI = ROOT / "carbonado-hip" / "src" / "ffi_paudit.rs"
LIB_RS = ROOT / "carbonado-hip" / "src" / "lib.rs"
CSRC = ROOT / "carbonado_amd" / "csrc"

OK, INVALID_ARG, HASH_DECODE, NO_DEVICE = 0, 1, 4, 100
NAMES = {"chipp_abi_version", "chipp_root_table_len", "chipp_root_table_dev", "chipp_audit_scratch_len",
         "chipp_proof_bound", "chipp_verify_slices_dev", "chipp_extract_slices_dev", "chipp_verify_proofs_dev"}
# the fourteenth boundary; boundary.BOUNDARIES holds the first nine
MINE = B._boundary("chipp_", "paudit", _lib.PAUDIT_SIGNATURES, 8)
OLDER = B.BOUNDARIES + (B._boundary("chipf_", "fread", _lib.FREAD_SIGNATURES, 7),
                        B._boundary("chipq_", "qread", _lib.QREAD_SIGNATURES, 6),
                        B._boundary("chipk_", "kread", _lib.KREAD_SIGNATURES, 6),
                        B._boundary("chipg_", "gread", _lib.GREAD_SIGNATURES, 5))


def prototypes() -> dict:
    return B.prototypes(HEADER, "chipp_")


def test_exports_header_and_ctypes_are_one_set():
    protos = prototypes()
    assert set(protos) == NAMES and len(NAMES) == MINE.exports == 8
    exported = B.exported()
    assert set(protos) == B.exports_of(exported, MINE.prefix) == set(MINE.signatures)
    for name, (_, ps) in protos.items():
        assert len(MINE.signatures[name][1]) == len(ps), name
    assert _lib.lib().chipp_abi_version() == 1
    text = HEADER.read_text()
    assert "#define CHIPP_ABI_VERSION 1" in text and "#define CHIPP_NO_REQUEST 0xFFFFFFFFu" in text
    # every older boundary keeps its count; no prefix clashes, no shared name
    assert [b.exports for b in OLDER] == [62, 5, 6, 4, 4, 3, 10, 10, 8, 7, 6, 6, 5]
    for b in OLDER:
        assert len(B.exports_of(exported, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(MINE.prefix) and not MINE.prefix.startswith(b.prefix)
        assert not set(MINE.signatures) & set(b.signatures), b.prefix
    # the argument lists the header states
    reqs = ["d_req_stream", "d_index", "d_count", "nreq", "max_count"]
    tail = ["d_status", "d_scratch", "scratch_len", "stream"]
    content = ["d_content", "content_stride", "d_content_len"]
    proofs = ["d_proofs", "proof_stride", "d_proof_len"]
    names = lambda f: [n for n, _ in protos[f][1]]  # noqa: E731
    assert names("chipp_root_table_dev") == ["content_len", "d_hash", "nroots", "d_table", "table_len", "info", "stream"]
    assert names("chipp_audit_scratch_len") == ["info_max_chunks", "nreq", "max_count"]
    assert names("chipp_proof_bound") == ["max_chunks", "max_count"]
    assert names("chipp_verify_slices_dev") == ["d_table", "info"] + reqs + content + tail
    assert names("chipp_extract_slices_dev") == ["d_table", "info"] + reqs + proofs + tail
    assert names("chipp_verify_proofs_dev") == ["d_roots", "root_info"] + reqs + proofs + content + tail
    assert ctypes.sizeof(_lib.RootInfo) == 32 and ctypes.sizeof(_lib.TableInfo) == 32


def test_ffi_paudit_declares_every_prototype_with_matching_types():
    B.assert_ffi_matches(B.ffi_declarations(FFI, "chipp_"), prototypes())
    text = B.ffi_text(FFI)
    assert re.search(r"pub const CHIPP_ABI_VERSION: c_int = 1;", text)
    assert re.search(r"pub const CHIPP_NO_REQUEST: u32 = 0xFFFF_FFFF;", text)
    m = re.search(r"#\[repr\(C\)\][^{]*pub struct chipp_root_info \{([^}]*)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("nroots", "u64"), ("max_chunks", "u64"),
                                                                ("reserved", "[u64; 2]")]
    header = RS._strip_comments(HEADER.read_text())
    body = re.search(r"typedef struct chipp_root_info \{([^}]*)\}", header, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+(?:\[\d+\])?);", body) == ["nroots", "max_chunks", "reserved[2]"]


WRAPPERS = (("root_table_len", "root_table", ("chipp_root_table_len",)),
            ("root_table", "root_table", ("chipp_root_table_dev",)),
            ("planned_audit_scratch_len", "planned_audit_scratch", ("chipp_audit_scratch_len",)),
            ("proof_bound", "proof_bound", ("chipp_proof_bound",)),
            ("verify_slices_planned", "verify_slices_planned", ("chipp_verify_slices_dev",)),
            ("extract_slices_planned", "extract_slices_planned", ("chipp_extract_slices_dev",)),
            ("verify_slice_proofs_planned", "verify_slice_proofs_planned", ("chipp_verify_proofs_dev",)))


def test_lib_rs_and_device_module_have_the_wrappers():
    lib = RS._strip_comments(LIB_RS.read_text())
    src = (ROOT / "carbonado_amd" / "device.py").read_text()
    assert re.search(r"^mod ffi_paudit;", lib, flags=re.M) and "chipp_abi_version" in lib
    assert re.search(r"^class RootTable:", src, flags=re.M)
    for rust_fn, py_fn, calls in WRAPPERS:
        m = re.search(rf"\npub fn {rust_fn}\(", lib)
        assert m, rust_fn
        body = lib[m.end():lib.index("\n}\n", m.end())]
        assert re.search(rf"^def {py_fn}\(", src, flags=re.M), py_fn
        for call in calls:
            assert f"ffi_paudit::{call}(" in body, (rust_fn, call)
            assert f"{call}(" in src, call


# never dereferenced: the checks come first
TAB, REQ, IDX, CNT, OUT, PRF = 0x79000000, 0x7A000000, 0x7A100000, 0x7A200000, 0x40000000, 0x50000000
CLEN, PLEN, STAT, SCR, HASH = 0x7A300000, 0x7A400000, 0x7A500000, 0x78000000, 0x70000000


def _last():
    import torch
    return NO_DEVICE if not torch.cuda.is_available() else None


def _u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs)


def test_table_scratch_and_bound_lengths():
    L = _lib.lib()
    assert L.chipp_root_table_len(0) == 0 and L.chipp_root_table_len(1 << 32) == 0
    for n in (1, 3, 6, 7, 1024):
        size = L.chipp_root_table_len(n)
        assert size % 16 == 0 and size >= 40 * n and L.chipp_root_table_len(n + 7) > size
    # 8 + 64 P + 1024 max_count, P = qread::slice_parents_bound: at most 2 + ((w - 1) >> L) parents per level
    assert L.chipp_proof_bound(1, 1) == 8 + 1024 and L.chipp_proof_bound(2, 1) == 8 + 64 + 1024
    assert L.chipp_proof_bound(1024, 1) == 8 + 64 * 19 + 1024 and L.chipp_proof_bound(66, 3) == 8 + 64 * 13 + 3072
    assert L.chipp_proof_bound(1024, 0) == 0 and L.chipp_proof_bound(1024, (1 << 53) + 1) == 0
    for mc, w in ((1, 1), (66, 3), (1024, 8), (1 << 20, 70)):
        b = L.chipp_proof_bound(mc, w)
        assert L.chipp_proof_bound(2 * mc + 1, w) >= b and L.chipp_proof_bound(mc, w + 1) >= b + 1024
    for nreq, w in ((1, 1), (1024, 1), (16384, 1), (65, 70)):
        s = L.chipp_audit_scratch_len(1024, nreq, w)
        assert s and s % 16 == 0 and s >= 72 * nreq and L.chipp_audit_scratch_len(1024, nreq + 64, w) > s
        assert L.chipp_audit_scratch_len(1 << 30, nreq, w + 5) == s  # the capacity sizes the grids, not the scratch
    for bad in ((1024, 1 << 31, 1), (1024, 16, 0), (1024, 16, (1 << 53) + 1), (1 << 20, 1 << 30, 64)):
        assert L.chipp_audit_scratch_len(*bad) == 0, bad
    assert L.chipp_audit_scratch_len(1024, 16, 1 << 53) > 0  # no request selects more chunks than its stream has
    assert L.chipp_audit_scratch_len(1024, 0, 1) % 16 == 0


def test_root_table_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    need = L.chipp_root_table_len(3)
    n3, over = [0, 5000, 1 << 62], [0, (1 << 62) + 1, 5]

    def call(ns=n3, hashes=HASH, table=TAB, table_len=need, nroots=3, arrays=True, info=True):
        out = _lib.RootInfo(9, 9, (9, 9))
        rc = L.chipp_root_table_dev(_u64(ns) if arrays else None, hashes, nroots, table, table_len,
                                    ctypes.byref(out) if info else None, None)
        return rc, (out.nroots, out.max_chunks, out.reserved[0], out.reserved[1])

    def rc(**kw):
        code, got = call(**kw)
        assert code == OK or got == (0, 0, 0, 0)  # nothing is reported of a table that was not made
        return code

    assert call(info=False)[0] == INVALID_ARG
    assert rc(arrays=False) == INVALID_ARG and rc(table=None) == INVALID_ARG and rc(table=TAB + 8) == INVALID_ARG
    assert rc(nroots=1 << 32, table_len=1 << 60) == INVALID_ARG
    assert rc(ns=over) == INVALID_ARG and rc(table_len=need - 1) == INVALID_ARG
    assert rc(hashes=None) == HASH_DECODE
    # the order: a NULL hash is reported behind every INVALID_ARG
    assert rc(hashes=None, table_len=need - 1) == INVALID_ARG and rc(hashes=None, ns=over) == INVALID_ARG
    assert rc(hashes=None, table=TAB + 8) == INVALID_ARG
    if last:
        assert rc() == last


def test_call_argument_errors_in_their_order():
    L = _lib.lib()
    last = _last()
    info_h, info_r = _lib.TableInfo(3, 66, 1024, 0), _lib.RootInfo(3, 66)
    need = L.chipp_audit_scratch_len(66, 6, 3)
    pb = -(-L.chipp_proof_bound(66, 3) // 16) * 16

    def call(kind, table=TAB, info=True, rs=REQ, idx=IDX, cnt=CNT, nreq=6, max_count=3, out=OUT, cs=3072, clen=CLEN,
             prf=PRF, ps=pb, plen=PLEN, stat=STAT, scratch=SCR, scratch_len=need):
        if kind == "verify":
            return L.chipp_verify_slices_dev(table, ctypes.byref(info_h) if info else None, rs, idx, cnt, nreq,
                                             max_count, out, cs, clen, stat, scratch, scratch_len, None)
        if kind == "extract":
            return L.chipp_extract_slices_dev(table, ctypes.byref(info_h) if info else None, rs, idx, cnt, nreq,
                                              max_count, prf, ps, plen, stat, scratch, scratch_len, None)
        return L.chipp_verify_proofs_dev(table, ctypes.byref(info_r) if info else None, rs, idx, cnt, nreq,
                                         max_count, prf, ps, plen, out, cs, clen, stat, scratch, scratch_len, None)

    uses = {"verify": ("out", "clen"), "extract": ("prf", "plen"), "proofs": ("out", "clen", "prf", "plen")}
    for kind in ("verify", "extract", "proofs"):
        rc = lambda **kw: call(kind, **kw)  # noqa: E731
        assert rc(nreq=0) == OK
        assert rc(nreq=0, table=None, info=False, rs=None, idx=None, cnt=None, out=None, clen=None, prf=None, plen=None,
                  stat=None, scratch=None, max_count=0, cs=7, ps=7, scratch_len=0) == OK
        for name in ("table", "rs", "idx", "cnt", "stat", "scratch") + uses[kind]:
            assert rc(**{name: None}) == INVALID_ARG, (kind, name)
        assert rc(info=False) == INVALID_ARG
        assert rc(nreq=1 << 31, scratch_len=1 << 60) == INVALID_ARG
        assert rc(max_count=0) == INVALID_ARG
        assert rc(max_count=(1 << 53) + 1, cs=1 << 58, ps=1 << 58, scratch_len=1 << 60) == INVALID_ARG
        has_content, has_proofs = "out" in uses[kind], "prf" in uses[kind]
        if has_content:
            assert rc(cs=3080) == INVALID_ARG and rc(cs=3056) == INVALID_ARG and rc(max_count=4) == INVALID_ARG
            assert rc(cs=1 << 62) == INVALID_ARG                    # a slot address would wrap
            assert rc(out=OUT + 8) == INVALID_ARG
        if has_proofs:
            assert rc(ps=pb + 8) == INVALID_ARG and rc(ps=pb - 16) == INVALID_ARG and rc(ps=1 << 62) == INVALID_ARG
            assert rc(prf=PRF + 8) == INVALID_ARG
            assert rc(max_count=4, cs=4096) == INVALID_ARG           # the proof bound grew with it
        assert rc(scratch=SCR + 8) == INVALID_ARG and rc(table=TAB + 8) == INVALID_ARG
        wide = dict(nreq=1 << 30, max_count=66, cs=66 * 1024, ps=-(-L.chipp_proof_bound(66, 66) // 16) * 16)
        assert rc(**wide, scratch_len=1 << 60) == INVALID_ARG       # 2^36 work items
        assert rc(scratch_len=need - 1) == INVALID_ARG
        # the order: the strides before the alignment, the alignment before the bounds, the bounds before the scratch
        assert rc(max_count=0, nreq=1 << 31) == INVALID_ARG and rc(**wide, scratch=SCR + 8, scratch_len=0) == INVALID_ARG
        if last:
            assert rc() == last and rc(cs=4096, ps=pb + 64, scratch_len=need + 5) == last


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return B.build_check(tmp_path_factory, "paudit_plan_check.cpp", include=[CSRC])


@pytest.mark.parametrize("seed", ["1", "0xBEEF"])
def test_paudit_plan_under_asan_ubsan(plan_check, seed):
    """The plan kernel's text on the host against audit::plan_verify and
    audit::plan_extract record for record, P and chipp_proof_bound against the
    true counts (exhaustively for N <= 256, w <= 8), the item -> (request, slot)
    arithmetic over every true work item, and the order of the host checks."""
    out = B.run_check(plan_check, seed, timeout=300)
    assert out.strip().splitlines()[-1] == "0 failures"


def test_paudit_bench_dry_run():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "paudit_bench.py"), "--dry"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["tool"] == "paudit_bench" and res["dry_run"] is True
    assert res["streams"] == 1024 and res["content_bytes"] == 1 << 20 and res["slice_bytes"] == 1024
    assert res["audit_1"]["requests"] == 1024 and res["audit_16"]["requests"] == 16384
    assert res["audit_16"]["parent_slots"] == 19 and res["audit_16"]["proof_stride"] == 2256
    assert res["audit_16"]["scratch_bytes"] == 16384 * 72 > res["audit_1"]["scratch_bytes"] > 0
    assert res["audit_16"]["scratch_bytes"] < res["audit_16"]["host_planned_scratch_bytes"]
    assert res["launches"] == {"verify": 4, "extract": 2, "verify_proofs": 4}
    assert res["uploads_per_call"] == 0 and res["memsets_per_call"] == 0
    assert res["table_bytes"] == _lib.lib().chipq_stream_table_len(1024)
    assert res["root_table_bytes"] == _lib.lib().chipp_root_table_len(1024)
