"""What the CPU tests of the extension boundaries (tests/test_*_cpu.py) share:
the table of every boundary, the parsers of a header's prototypes and of an
ffi_*.rs file's declarations, the library's exported symbols, and the build
and run of a stand-alone check program under ASan + UBSan."""
import os
import re
import shutil
import subprocess
from collections import namedtuple
from pathlib import Path

import pytest

import test_rust_shim as RS
from carbonado_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
RUST_SRC = ROOT / "carbonado-hip" / "src"
LIB_RS = RUST_SRC / "lib.rs"

Boundary = namedtuple("Boundary", "prefix header ffi signatures exports")


def _boundary(prefix, stem, signatures, exports):
    header = "carbonado_hip.h" if stem is None else f"carbonado_hip_{stem}.h"
    ffi = "ffi.rs" if stem is None else f"ffi_{stem}.rs"
    return Boundary(prefix, INCLUDE / header, RUST_SRC / ffi, signatures, exports)


# every boundary in the order it was added: prefix, header, ffi file, _lib's signature table, exported symbols
BOUNDARIES = (
    _boundary("chip_", None, _lib.SIGNATURES, 62),
    _boundary("chipx_", "ext", _lib.EXT_SIGNATURES, 5),
    _boundary("chipa_", "audit", _lib.AUDIT_SIGNATURES, 6),
    _boundary("chipr_", "repair", _lib.REPAIR_SIGNATURES, 4),
    _boundary("chipd_", "read", _lib.READ_SIGNATURES, 4),
    _boundary("chipv_", "vread", _lib.VREAD_SIGNATURES, 3),
    _boundary("chipe_", "ecies", _lib.ECIES_SIGNATURES, 10),
    _boundary("chips_", "snap", _lib.SNAP_SIGNATURES, 10),
    _boundary("chipc_", "cread", _lib.CREAD_SIGNATURES, 8),
)


def boundary(prefix: str) -> Boundary:
    return next(b for b in BOUNDARIES if b.prefix == prefix)


def older(prefix: str) -> tuple:
    """The boundaries added before this one."""
    return BOUNDARIES[:BOUNDARIES.index(boundary(prefix))]


def prototypes(header: Path, prefix: str) -> dict:
    """name -> (return type, [(parameter, type)]) of a header's prototypes, types in Rust's spelling."""
    text = RS._strip_comments(header.read_text())
    api = prefix.rstrip("_").upper() + "_API"
    protos = {}
    for ret, name, params in re.findall(rf"{api}\s+([^;{{}}()]*?)\b({prefix}\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
        ps = []
        params = " ".join(params.split())
        if params and params != "void":
            for p in params.split(","):
                m = re.match(r"(.*?)(\w+)$", p.strip())
                ps.append((m.group(2), RS.c_to_rust(m.group(1))))
        protos[name] = (RS.c_to_rust(ret), ps)
    return protos


def ffi_text(ffi: Path) -> str:
    return RS._strip_comments(ffi.read_text())


def ffi_declarations(ffi: Path, prefix: str) -> dict:
    """name -> (return type, [(parameter, type)]) of the extern "C" blocks of an ffi_*.rs file."""
    decls = {}
    for block in re.findall(r'extern\s+"C"\s*\{(.*?)\n\}', ffi_text(ffi), flags=re.S):
        for name, params, ret in re.findall(rf"pub\s+fn\s+({prefix}\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+?))?\s*;", block,
                                            flags=re.S):
            assert name not in decls
            ps = [tuple(" ".join(s.split()) for s in p.split(":", 1))
                  for p in filter(None, (x.strip() for x in " ".join(params.split()).split(",")))]
            decls[name] = (" ".join(ret.split()) if ret else "", ps)
    return decls


def assert_ffi_matches(decls: dict, protos: dict):
    assert set(decls) == set(protos)
    for name, (cret, cps) in protos.items():
        rret, rps = decls[name]
        assert cret == rret, name
        assert [t for _, t in cps] == [t for _, t in rps], name
        assert [n for n, _ in cps] == [n for n, _ in rps], name


def exported() -> set:
    """The symbols the library defines (nm -D)."""
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def exports_of(symbols: set, prefix: str) -> set:
    return {s for s in symbols if s.startswith(prefix)}


def assert_one_set(protos: dict, symbols: set, prefix: str):
    """A boundary's header, its exported symbols and its ctypes table name the same
    functions, with as many parameters each."""
    mine = boundary(prefix)
    assert set(protos) == exports_of(symbols, prefix) == set(mine.signatures) and len(protos) == mine.exports
    for name, (_, ps) in protos.items():
        assert len(mine.signatures[name][1]) == len(ps), name


def assert_older_keep_their_sets(symbols: set, prefix: str):
    """Every boundary added before `prefix` still exports its count, shares no
    name with it in _lib's tables, and neither prefix is a prefix of the other."""
    mine = boundary(prefix)
    for b in older(prefix):
        assert len(exports_of(symbols, b.prefix)) == b.exports, b.prefix
        assert not b.prefix.startswith(prefix) and not prefix.startswith(b.prefix)
        assert not set(mine.signatures) & set(b.signatures), b.prefix


def build_check(tmp_path_factory, source: str, include=(), libs=(), extra_sources=()):
    """tests/<source> (and extra_sources) into a stand-alone program under ASan + UBSan; its path."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    stem = Path(source).stem
    exe = tmp_path_factory.mktemp(stem + "_asan") / stem
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", str(ROOT / "tests" / source), *(str(s) for s in extra_sources),
           "-I" + str(INCLUDE), *("-I" + str(d) for d in include), "-o", str(exe), *("-l" + lib for lib in libs)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def run_check(exe, *args, timeout=120) -> str:
    """Run a check program; it must exit 0.  Its output."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout
