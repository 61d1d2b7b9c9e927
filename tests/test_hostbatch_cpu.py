"""CPU tests of the planning arithmetic of encode() / decode() from host memory
(carbonado_amd/csrc/hostbatch_plan.hpp): the header as a stand-alone program
under ASan + UBSan (tests/hostbatch_plan_check.cpp), and the region end it
computes against bench.py's own statement of it."""
import re
import sys
from pathlib import Path

import pytest

import boundary as B

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "carbonado_amd" / "csrc"
sys.path.insert(0, str(ROOT))

# what dec_geom gives a level-12 header whose stream is three bytes short
# (CHIP_ERR_BAO_TRUNCATED); tests/test_gpu_pipeline.py expects it of the host batch
HEADER_SHORT_STATUS = 6

CHUNK_COUNTS = [2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 16384]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    # host_stage_max reads the snappy frame bound from the host stages themselves
    exe = B.build_check(tmp_path_factory, "hostbatch_plan_check.cpp", include=[CSRC],
                        extra_sources=[CSRC / "host_snap.cpp"])
    return B.run_check(exe, timeout=300)


def test_hostbatch_plan_under_asan_ubsan(check_output):
    """Region geometry against a brute-force walk of the stream, slice sizing as
    a literal table, encode's bounds and dec_geom's statuses."""
    assert check_output.strip().splitlines()[-1] == "0 failures"
    assert "FAIL" not in check_output
    assert re.findall(r"^header_short_status (\d+)$", check_output, flags=re.M) == [str(HEADER_SHORT_STATUS)]


def test_region_end_is_bench_pys(check_output):
    """t0 of (1024 N, N / 2), the end of the data region of a Zfec|Bao stream of N
    chunks, is bench.bao_data_region_len(N): a statement of its own, tested
    against the oracle's stream in tests/test_bench_helpers.py."""
    import bench
    t0 = {int(n): int(v) for n, v in re.findall(r"^t0 (\d+) (\d+)$", check_output, flags=re.M)}
    assert sorted(t0) == CHUNK_COUNTS
    for n in CHUNK_COUNTS:
        assert t0[n] == bench.bao_data_region_len(n), n
