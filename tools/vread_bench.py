#!/usr/bin/env python3
"""Vouched byte-range reads of device-resident level-12 (Zfec|Bao) streams:
one chipv_read_ranges_dev call (include/carbonado_hip_vread.h) against the
unvouched call and against what a caller who needs vouched bytes had before it
(GPU only; not bench.py).  The sets, the damage and the box discipline are
those of tools/read_bench.py: --streams streams of 1 MiB objects in one buffer,
one random 4 KiB object range per stream (and 16 per stream).

  intact    read, read_again  chipd_read_ranges_dev, twice in every round: the
                              spread between repeated runs of the same call
            vread             chipv_read_ranges_dev, flags 0: two more launches
                              (8 against 6), both gated, no more hashing
  damaged   1 stream in 64 with a flipped bit in a primary chunk inside its
            range:
            vread             the damaged ranges are rebuilt and every rebuilt
                              chunk hashed against its stored CV: vouch 1
            read              chipd_read_ranges_dev on the same damage: the
                              price of the guarantee is vread / read
            scrub_verify      chipr_scrub_ragged_dev into a second buffer, then
                              chipa_verify_slices_dev: the only way to vouched
                              bytes before this call
  sixteen   read / vread with 16 ranges per stream

Before anything is timed every form's bytes are compared with the clean
objects, and the damaged reads must come out status 0, vouch 1, all others
vouch 0.  Timing as in read_bench.py: HIP events around each call, the forms
alternating within one process for --reps rounds after 3 warm-ups, medians and
min-max in ms.  Prints one JSON line (and writes it to --out).

--dry-run needs no device: it lays out the same three request sets on the
host (chipd_read_layout, both scratch lengths) and prints the same JSON shape
with null timings."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

LEVEL = 12
OBJ = 1 << 20
RANGE = 4096
CASES = (("intact", 1, 0, 0), ("damaged_1_in_64", 1, 64, 1), ("sixteen_per_stream", 16, 0, 2))  # name, per, every, seed +


def dry_run(args):
    """The three sets' requests, laid out on the host; no device is touched."""
    import ctypes

    from carbonado_amd import _lib
    L = _lib.lib()
    C, pad = OBJ // 4, 41
    res = {"tool": "vread_bench", "dry_run": True, "level": LEVEL, "seed": args.seed, "streams": args.streams,
           "object_bytes": OBJ - pad, "range_bytes": RANGE, "reps": args.reps}
    for name, per, every, ds in CASES:
        count = args.streams
        rng = np.random.default_rng(args.seed + ds)
        rs = np.repeat(np.arange(count, dtype=np.uint32), per)
        start = rng.integers(0, 4 * C - pad - RANGE, count * per).astype(np.uint64)
        rlen = np.full(count * per, RANGE, dtype=np.uint64)
        cl, pd = np.full(count, C, dtype=np.uint32), np.full(count, pad, dtype=np.uint32)
        off, ln = np.zeros(count * per, dtype=np.uint64), np.zeros(count * per, dtype=np.uint64)
        total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
        p32, p64 = (lambda a: a.ctypes.data_as(_lib.c_u32p)), (lambda a: a.ctypes.data_as(_lib.c_u64p))
        rc = L.chipd_read_layout(p32(cl), p32(pd), count, p32(rs), p64(start), p64(rlen), count * per, 16, p64(off), p64(ln),
                                 ctypes.byref(total), ctypes.byref(nseg))
        assert rc == 0 and (ln == RANGE).all() and total.value == RANGE * count * per
        need, old = L.chipv_read_scratch_len(count * per, nseg.value), L.chipd_read_scratch_len(count * per, nseg.value)
        assert need >= old and need % 16 == 0
        res[name] = {"requests": count * per, "segments": nseg.value, "damaged": len(range(0, count, every)) if every else 0,
                     "scratch_bytes": need, "scratch_bytes_unvouched": old, "vread": None, "read": None}
    line = json.dumps(res)
    print(line)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry-run", action="store_true", help="no device: lay the request sets out on the host")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry_run:
        return dry_run(args)

    import torch

    import read_bench as RB
    from bench import ClockSampler
    from carbonado_amd import _lib
    from carbonado_amd import device as D
    ptr, vp = RB.ptr, RB.vp

    class Set(RB.Set):
        """read_bench's set with the vouched call's buffers beside the unvouched one's."""

        def __init__(self, L, count, per, every, seed):
            super().__init__(L, count, per, every, seed)
            self.vouch = torch.zeros(self.nreq, dtype=torch.int32, device="cuda")
            self.vscratch = D.vread_scratch(self.nreq, self.nseg)

        def vread(self):
            rc = self.L.chipv_read_ranges_dev(vp(self.buf), ptr(self.in_off), ptr(self.in_len), vp(self.hashes),
                                              ptr(self.pad), ptr(self.cl), self.count, ptr(self.rs), ptr(self.start),
                                              ptr(self.rlen), self.nreq, vp(self.content), ptr(self.coff), ptr(self.clen),
                                              vp(self.status), vp(self.used), vp(self.vouch), 0, vp(self.vscratch),
                                              self.vscratch.numel(), None)
            assert rc == 0, rc

        def check_vread(self, sample):
            """check_read's checks through the vouched call, and the vouch words."""
            plain, self.read = self.read, self.vread
            try:
                self.vouch.fill_(-1)
                rebuilt = self.check_read(sample)
            finally:
                self.read = plain
            vouch, hurt = self.vouch.cpu().numpy(), set(self.damaged)
            for r in range(self.nreq):
                hit = r % self.per == 0 and r // self.per in hurt
                assert int(vouch[r]) == (1 if hit else 0), (r, int(vouch[r]))
            return rebuilt

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "vread_bench", "level": LEVEL, "seed": args.seed, "streams": args.streams, "object_bytes": OBJ - 41,
           "range_bytes": RANGE, "reps": args.reps,
           "timing": "HIP events around each call, host_median_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams

    s = Set(L, S, 1, 0, args.seed)
    sample = range(0, s.nreq, max(1, s.nreq // 256))
    assert s.check_read(sample) == 0 and s.check_vread(sample) == 0
    r = res["intact"] = {"requests": s.nreq, "segments": int(s.nseg),
                         **RB.time_forms({"read": s.read, "vread": s.vread, "read_again": s.read}, args.reps)}
    lo = min(r["read"]["min_ms"], r["read_again"]["min_ms"])
    hi = max(r["read"]["max_ms"], r["read_again"]["max_ms"])
    r["read_spread_ms"] = round(hi - lo, 4)
    r["read_medians_apart_ms"] = round(abs(r["read"]["median_ms"] - r["read_again"]["median_ms"]), 4)
    r["vread_minus_read_ms"] = round(r["vread"]["median_ms"] - r["read"]["median_ms"], 4)
    r["vread_over_read"] = round(r["vread"]["median_ms"] / r["read"]["median_ms"], 3)
    r["vread_within_read_spread"] = lo <= r["vread"]["median_ms"] <= hi
    r["extra_launches"] = 2
    r["per_extra_launch_ms"] = round(r["vread_minus_read_ms"] / 2, 4)
    del s
    torch.cuda.empty_cache()

    s = Set(L, S, 1, 64, args.seed + 1)
    sample = sorted(set(range(0, s.nreq, max(1, s.nreq // 128))) | set(s.damaged))
    assert s.check_read(sample) == len(s.damaged) and s.check_vread(sample) == len(s.damaged)
    picked, hurt = set(sample), set(s.damaged)
    segs = [g for g, (rq, _, _, _) in enumerate(s.seg_of) if rq in picked]
    s.check_verify(segs, s.scrub_verify)
    assert [int(x) for x in s.s_status] == [0 if j in hurt else 12 for j in range(S)]
    r = res["damaged_1_in_64"] = {"requests": s.nreq, "damaged": len(s.damaged), "damaged_reads_vouch": 1,
                                  **RB.time_forms({"vread": s.vread, "scrub_verify": s.scrub_verify, "read": s.read},
                                                  args.reps)}
    r["scrub_verify_over_vread"] = round(r["scrub_verify"]["median_ms"] / r["vread"]["median_ms"], 2)
    r["vread_over_read"] = round(r["vread"]["median_ms"] / r["read"]["median_ms"], 3)
    del s
    torch.cuda.empty_cache()

    s = Set(L, S, 16, 0, args.seed + 2)
    sample = range(0, s.nreq, max(1, s.nreq // 256))
    assert s.check_read(sample) == 0 and s.check_vread(sample) == 0
    r = res["sixteen_per_stream"] = {"requests": s.nreq, "segments": int(s.nseg),
                                     **RB.time_forms({"read": s.read, "vread": s.vread}, args.reps)}
    r["vread_over_read"] = round(r["vread"]["median_ms"] / r["read"]["median_ms"], 3)
    del s

    res["clocks"] = clocks.stop()
    res["intact_vread_within_read_spread"] = res["intact"]["vread_within_read_spread"]
    res["damaged_vread_beats_scrub_verify"] = res["damaged_1_in_64"]["scrub_verify_over_vread"] > 1
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
