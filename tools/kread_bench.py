#!/usr/bin/env python3
"""Plaintext ranged reads of level-13 streams planned on the device against the
host-planned ones, on cread_bench.py's set (GPU only; not bench.py): --streams
level-13 streams whose envelopes have 1 MiB - 41 bytes in one buffer, random
4 KiB plaintext ranges, one per stream and 16 per stream, intact and with 1
stream in 64 damaged inside its first range.

  planned     chipk_read_ranges_dev (include/carbonado_hip_kread.h): the
              requests are device arrays, the keys are resident, no upload
  replay      one captured chipk_read_ranges_dev call, replayed
  host        chipc_read_ranges_dev over the same requests: the host plans,
              uploads two tables and expands every key
  key_table   chipk_key_table_dev, the once-per-set key setup (timed apart)

Before anything is timed the planned call's and the replay's bytes are compared
with the objects, all of them, and its words with the host-planned call's.  A
time is between two HIP events around the call (no call synchronises);
host_*_ms is the host clock around the same call.  3 warm-ups, the forms
alternating within one process for --reps rounds; medians and min-max in ms,
the GPU's clocks sampled meanwhile.  Prints one JSON line (and writes it to
--out) with the two conditions the call was built on: at 16 ranges per stream
its median is below the host-planned call's MINIMUM, and at one range per
stream it is not above that call's maximum.

--dry needs no device: the capacity, the table and scratch sizes and the launch
counts of both request sets through the library's host-only calls."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

LEVEL = 13
ENV = (1 << 20) - 41        # the envelope, as in cread_bench.py
PLAIN = ENV - 97
RANGE = 4096
SECRET = bytes(range(1, 33))
LAUNCHES = {"rewrite": 1, "plan": 4, "vouched_read": 8, "keystream": 1, "total": 14}
CASES = (("intact", 0), ("damaged_1_in_64", 64))


def requests(count, per, seed):
    rng = np.random.default_rng(seed)
    rs = np.repeat(np.arange(count, dtype=np.uint32), per)
    start = rng.integers(0, PLAIN - RANGE, count * per).astype(np.uint64)
    return rs, start, np.full(count * per, RANGE, dtype=np.uint64)


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    S, C = args.streams, (1 << 20) // 4
    info = _lib.TableInfo(S, 8 * C // 1024, C, 0)
    res = {"tool": "kread_bench", "dry_run": True, "level": LEVEL, "seed": args.seed, "streams": S,
           "envelope_bytes": ENV, "object_bytes": PLAIN, "range_bytes": RANGE, "reps": args.reps,
           "max_chunks": info.max_chunks, "min_shard": info.min_shard,
           "stream_table_bytes": L.chipq_stream_table_len(S), "key_table_bytes": L.chipk_key_table_len(S),
           "launches": LAUNCHES, "key_table_launches": 2, "uploads_per_read": 0, "memsets_per_read": 0}
    for per in (1, 16):
        nreq = S * per
        res[f"read_{per}"] = {
            "requests": nreq, "max_len": RANGE, "content_stride": RANGE,
            "scratch_bytes": L.chipk_read_scratch_len(ctypes.byref(info), nreq, RANGE),
            "keystream_waves": nreq * -(-(RANGE // 16) // 127),
            "damaged_streams": len(range(0, S, 64))}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry", action="store_true", help="no device: sizes and launch counts only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)

    import torch

    import read_bench as RB
    from bench import ClockSampler
    from carbonado_amd import _lib
    from carbonado_amd import device as D
    from oracle import oracle as O
    from qread_bench import time_forms

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "kread_bench", "level": LEVEL, "seed": args.seed, "streams": args.streams, "envelope_bytes": ENV,
           "object_bytes": PLAIN, "range_bytes": RANGE, "reps": args.reps, "launches": LAUNCHES,
           "uploads_per_read": 0, "memsets_per_read": 0,
           "timing": "HIP events around each call, host_*_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams
    pub = O.c_public_key(SECRET)
    sizes, pitch = [PLAIN] * S, 1 << 20
    in_off = [o * pitch for o in range(S)]
    off, slen, total = D.ragged_layout(12, [ENV] * S, 256)
    ptr, vp = RB.ptr, RB.vp
    p8 = lambda a: a.ctypes.data_as(_lib.c_u8p)  # noqa: E731
    a64, a32 = (lambda x: np.ascontiguousarray(x, dtype=np.uint64)), (lambda x: np.ascontiguousarray(x, dtype=np.uint32))

    for per in (1, 16):
        for name, every in CASES:
            seed = args.seed + per + every
            torch.manual_seed(seed)
            inp = torch.randint(0, 256, (S * pitch,), dtype=torch.uint8, device="cuda")
            buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
            hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
            olen, infos = D.encode_ragged_ecies(LEVEL, pub, inp, in_off, sizes, buf, off, hashes,
                                                D.ecies_ragged_scratch(LEVEL, sizes))
            torch.cuda.synchronize()
            pad, cl = [i.padding_len for i in infos], [i.chunk_len for i in infos]
            C, spc = cl[0], cl[0] // 1024
            rs, start, rlen = requests(S, per, seed)
            nreq = S * per
            damaged = list(range(0, S, every)) if every else []
            if damaged:  # a bit of the primary chunk that holds the first byte of the stream's first range
                at = []
                for k, j in enumerate(damaged):
                    x = int(start[j * per]) + 97
                    at.append(off[j] + RB.chunk_off(x // C * spc + x % C // 1024, 8 * spc) + 17 * k % 1024)
                buf[torch.tensor(at, dtype=torch.int64, device="cuda")] ^= 0x10
            keys, ivs, kstat = D.stream_keys(SECRET, buf, off, olen, hashes, pad, cl, D.stream_keys_scratch(S))
            assert not kstat.any()
            keys, ivs, kstat = np.ascontiguousarray(keys), np.ascontiguousarray(ivs), a32(kstat)

            # the host-planned call: arrays converted once, no wrapper in between
            coff, clen, ctotal, nseg = D.plain_read_layout(cl, pad, rs, start, rlen)
            h_content = torch.zeros(ctotal + 16, dtype=torch.uint8, device="cuda")
            h_status, h_used, h_vouch = (torch.zeros(nreq, dtype=torch.int32, device="cuda") for _ in range(3))
            h_scratch = D.plain_read_scratch(nreq, nseg, S)
            n_off, n_len, n_pad, n_cl, n_coff, n_clen = a64(off), a64(olen), a32(pad), a32(cl), a64(coff), a64(clen)

            def host():
                rc = L.chipc_read_ranges_dev(p8(keys), p8(ivs), ptr(kstat), vp(buf), ptr(n_off), ptr(n_len), vp(hashes),
                                             ptr(n_pad), ptr(n_cl), S, ptr(rs), ptr(start), ptr(rlen), nreq,
                                             vp(h_content), ptr(n_coff), ptr(n_clen), vp(h_status), vp(h_used),
                                             vp(h_vouch), 0, vp(h_scratch), h_scratch.numel(), None)
                assert rc == 0, rc

            # the device-planned call: the two tables once, the requests as device tensors
            table = D.stream_table(buf, off, olen, hashes, pad, cl)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ktab = D.key_table(keys, ivs, kstat)
            ktab_host_ms = (time.perf_counter() - t0) * 1e3
            b.record()
            b.synchronize()
            ktab_ms = a.elapsed_time(b)
            dev = lambda x, dt: torch.from_numpy(x.astype(dt)).cuda()  # noqa: E731
            d_rs, d_start, d_len = dev(rs, "int32"), dev(start, "int64"), dev(rlen, "int64")
            content = torch.zeros(nreq * RANGE, dtype=torch.uint8, device="cuda")
            d_clen = torch.zeros(nreq, dtype=torch.int64, device="cuda")
            status, used, vouch = (torch.zeros(nreq, dtype=torch.int32, device="cuda") for _ in range(3))
            scratch = D.planned_plain_read_scratch(table, nreq, RANGE)

            def planned():
                D.read_plain_ranges_planned(table, ktab, d_rs, d_start, d_len, RANGE, content, RANGE, d_clen, status,
                                            used, vouch, scratch)

            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                planned()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                planned()

            # every request's bytes against the objects, the words against the host-planned call's
            at = d_rs.to(torch.int64) * pitch + d_start
            want = inp[at[:, None] + torch.arange(RANGE, device="cuda")[None, :]]
            h_content.fill_(0x5A)
            host()
            torch.cuda.synchronize()
            got = h_content[torch.from_numpy(a64(coff).astype("int64")).cuda()[:, None] +
                            torch.arange(RANGE, device="cuda")[None, :]]
            assert int(h_status.count_nonzero()) == 0 and torch.equal(got, want), "host"
            for form, f in (("planned", planned), ("replay", graph.replay)):
                content.fill_(0xA5); status.fill_(-1); used.fill_(-1); vouch.fill_(-1); d_clen.fill_(-1)
                f()
                torch.cuda.synchronize()
                assert int(status.count_nonzero()) == 0 and bool((d_clen == RANGE).all()), form
                assert torch.equal(content.view(nreq, RANGE), want), form
                assert torch.equal(used, h_used) and torch.equal(vouch, h_vouch), form
            assert (int(vouch.count_nonzero()) > 0) == bool(damaged)

            r = {"requests": nreq, "segments": int(nseg), "damaged": len(damaged),
                 "scratch_bytes": scratch.numel(), "host_planned_scratch_bytes": h_scratch.numel(),
                 "key_table": {"ms": round(ktab_ms, 4), "host_ms": round(ktab_host_ms, 4), "bytes": ktab.table.numel()},
                 **time_forms({"planned": planned, "host": host, "replay": graph.replay}, args.reps)}
            r["planned_over_host"] = round(r["planned"]["median_ms"] / r["host"]["median_ms"], 3)
            r["replay_over_host"] = round(r["replay"]["median_ms"] / r["host"]["median_ms"], 3)
            res[f"read_{per}_{name}"] = r
            D.wipe_key_table(ktab)
            torch.cuda.synchronize()
            assert int(ktab.table.count_nonzero()) == 0
            del inp, buf, content, h_content, scratch, h_scratch, graph, table, ktab, want, got
            torch.cuda.empty_cache()

    res["clocks"] = clocks.stop()
    res["planned_median_below_host_min_at_16"] = all(
        res[k]["planned"]["median_ms"] < res[k]["host"]["min_ms"] for k in res if k.startswith("read_16_"))
    res["planned_median_not_above_host_max_at_1"] = all(
        res[k]["planned"]["median_ms"] <= res[k]["host"]["max_ms"] for k in res if k.startswith("read_1_"))
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
