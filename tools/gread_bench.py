#!/usr/bin/env python3
"""Plaintext ranged reads of level-14 and level-15 streams planned on the device
against the host-planned ones, on fread_bench.py's set (GPU only; not bench.py):
--streams streams of 1 MiB objects at 14 and at 15, each on the two corpora of
tools/snap_bench.py (mix40: every chunk compressed; random: every chunk stored
raw), random 4 KiB plaintext ranges, one per stream and 16 per stream, intact
and with 1 stream in 64 damaged inside the first frame of its first range.

  planned      chipg_read_ranges_dev (include/carbonado_hip_gread.h): the
               requests are device arrays, the frame indexes and the keys are
               resident, no upload
  replay       one captured chipg_read_ranges_dev call, replayed
  host         chipf_read_ranges_dev over the same requests: the host plans,
               re-checks every index, uploads its tables and expands every key
  frame_table  chipg_frame_table_dev, the once-per-set upload (timed apart)

Before anything is timed every form's bytes are compared with the objects, all
of them, and the planned words with the host-planned call's.  A time is between
two HIP events around the call (no call synchronises); host_*_ms is the host
clock around the same call.  3 warm-ups, the forms alternating within one
process for --reps rounds; medians and min-max in ms, the GPU's clocks sampled
meanwhile.  Prints one JSON line (and writes it to --out) with the three
conditions the call was built on, the yardstick being the host-planned call of
the same run: (a) on random data at 16 ranges per stream the planned median is
below the host-planned minimum; (b) in every other cell the planned median is
not above the host-planned maximum; (c) the planned call's host time is the
same at 1024 and 16384 requests (reported: the medians and their ratio).

--dry needs no device: the capacity, the table and scratch sizes and the launch
counts of both request sets through the library's host-only calls, for streams
of 16 raw frames (the random corpus)."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

SEG = 1 << 20
RANGE = 4096
FRAME = 65536
FRAMES = SEG // FRAME
SECRET = bytes(range(1, 33))
CORPORA = ("mix40", "random")
LAUNCHES = {"14": {"rewrite": 1, "plan": 4, "vouched_read": 8, "block": 1, "finish": 1, "total": 15},
            "15": {"rewrite": 1, "inner_rewrite": 1, "plan": 4, "vouched_read": 8, "keystream": 1, "block": 1, "finish": 1,
                   "total": 17}}
CASES = (("intact", 0), ("damaged_1_in_64", 64))
FCAP = (RANGE + FRAME - 2) // FRAME + 1


def requests(count, per, seed):
    rng = np.random.default_rng(seed)
    rs = np.repeat(np.arange(count, dtype=np.uint32), per)
    start = rng.integers(0, SEG - RANGE, count * per).astype(np.uint64)
    return rs, start, np.full(count * per, RANGE, dtype=np.uint64)


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    S = args.streams
    flen = 10 + FRAMES * (FRAME + 8)            # a random object's frame stream: 16 raw chunks
    res = {"tool": "gread_bench", "dry_run": True, "seed": args.seed, "streams": S, "object_bytes": SEG,
           "range_bytes": RANGE, "reps": args.reps, "frames_per_stream": FRAMES, "max_frame": FRAME + 8, "fcap": FCAP,
           "launches": LAUNCHES, "uploads_per_read": 0, "memsets_per_read": 0,
           "stream_table_bytes": L.chipq_stream_table_len(S), "key_table_bytes": L.chipk_key_table_len(S),
           "frame_table_bytes": L.chipg_frame_table_len(S, S * (FRAMES + 1))}
    for fmt in (14, 15):
        pad, chunk = ctypes.c_uint32(), ctypes.c_uint32()
        assert L.chip_calc_padding_len(flen + (97 if fmt == 15 else 0), 4, ctypes.byref(pad), ctypes.byref(chunk)) == 0
        info = _lib.TableInfo(S, 8 * chunk.value // 1024, chunk.value, 0)
        finfo = _lib.FrameInfo(S, S * (FRAMES + 1), FRAME + 8, fmt)
        r = res[f"level{fmt}"] = {"max_chunks": info.max_chunks, "min_shard": info.min_shard}
        for per in (1, 16):
            nreq = S * per
            r[f"read_{per}"] = {
                "requests": nreq, "max_len": RANGE, "content_stride": RANGE, "block_workgroups": nreq * FCAP,
                "staging_bytes": nreq * ((FCAP * (FRAME + 8) + 15) // 16 * 16),
                "scratch_bytes": L.chipg_read_scratch_len(ctypes.byref(info), ctypes.byref(finfo), nreq, RANGE),
                "damaged_streams": len(range(0, S, 64))}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--corpus", choices=CORPORA, help="this corpus only (a partial run: for a profiler)")
    ap.add_argument("--level", type=int, choices=(14, 15), help="this level only (a partial run)")
    ap.add_argument("--dry", action="store_true", help="no device: sizes and launch counts only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)

    import torch

    import read_bench as RB
    import snap_data as SD
    from bench import ClockSampler
    from carbonado_amd import _lib
    from carbonado_amd import device as D
    from carbonado_amd import encoding as E
    from fread_bench import layout
    from qread_bench import time_forms

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "gread_bench", "seed": args.seed, "streams": args.streams, "object_bytes": SEG, "range_bytes": RANGE,
           "reps": args.reps, "launches": LAUNCHES, "uploads_per_read": 0, "memsets_per_read": 0,
           "timing": "HIP events around each call, host_*_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams
    pub = E.public_key(SECRET)
    sizes, in_off = [SEG] * S, [o * SEG for o in range(S)]
    ptr, vp = RB.ptr, RB.vp
    p8 = lambda a: a.ctypes.data_as(_lib.c_u8p)  # noqa: E731
    a64, a32 = (lambda x: np.ascontiguousarray(x, dtype=np.uint64)), (lambda x: np.ascontiguousarray(x, dtype=np.uint32))
    dev = lambda x, dt: torch.from_numpy(x.astype(dt)).cuda()  # noqa: E731
    cells = {}

    for corpus in [args.corpus] if args.corpus else CORPORA:
        rng = np.random.default_rng(args.seed)
        rows = [np.frombuffer(SD.mix(SEG, 40, args.seed + i), dtype=np.uint8) if corpus == "mix40"
                else rng.integers(0, 256, SEG, dtype=np.uint8) for i in range(8)]
        host_rows = torch.empty((S, SEG), dtype=torch.uint8)
        for o in range(S):
            host_rows[o] = torch.from_numpy(rows[o % 8].copy())
        inp = host_rows.cuda().view(-1)
        del host_rows
        for fmt in [args.level] if args.level else (14, 15):
            shift = 97 if fmt == 15 else 0
            off, cap, total = D.snap_encode_layout(fmt, sizes, 256)
            buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
            hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
            olen, infos = D.encode_ragged_snap(fmt, inp, in_off, sizes, buf, off, hashes, D.snap_ragged_scratch(fmt, sizes),
                                               pubkey=pub if fmt == 15 else None)
            torch.cuda.synchronize()
            pad, cl = [i.padding_len for i in infos], [i.chunk_len for i in infos]
            keys = ivs = ktab = None
            if fmt == 15:
                keys, ivs, kstat = D.stream_keys(SECRET, buf, off, olen, hashes, pad, cl, D.stream_keys_scratch(S))
                assert not kstat.any()
                keys, ivs = np.ascontiguousarray(keys), np.ascontiguousarray(ivs)
            caps = FRAMES + 1
            idx_off = a64(np.arange(S) * caps)
            frame_off, nframes, istat, plain, ivouch = D.frame_index(fmt, buf, off, olen, hashes, pad, cl, idx_off,
                                                                     [caps] * S, D.frame_index_scratch(S, S * caps),
                                                                     keys=keys, ivs=ivs)
            assert not istat.any() and not ivouch.any() and (plain == SEG).all() and (nframes == FRAMES).all()
            frame_off, nframes, plain = a64(frame_off), a64(nframes), a64(plain)
            n_off, n_len, n_pad, n_cl = a64(off), a64(olen), a32(pad), a32(cl)
            pk, pv = (p8(keys), p8(ivs)) if fmt == 15 else (None, None)

            # the tables, once per set
            table = D.stream_table(buf, off, olen, hashes, pad, cl)
            if fmt == 15:
                ktab = D.key_table(keys, ivs, None)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            ftab = D.frame_table(fmt, cl, pad, frame_off, idx_off, nframes, plain)
            ftab_host_ms = (time.perf_counter() - t0) * 1e3
            b.record()
            b.synchronize()
            level = res[f"level{fmt}_{corpus}"] = {
                "stream_bytes": int(sum(olen)), "frame_stream_bytes": int(frame_off[caps - 1]),
                "max_frame": int(ftab.max_frame), "entries": int(ftab.nentries),
                "frame_table": {"ms": round(a.elapsed_time(b), 4), "host_ms": round(ftab_host_ms, 4),
                                "bytes": ftab.table.numel()}}
            C, spc = cl[0], cl[0] // 1024

            for per in (1, 16):
                for name, every in CASES:
                    rs, start, rlen = requests(S, per, args.seed + per + every)
                    nreq = S * per
                    damaged = list(range(0, S, every)) if every else []
                    at = []
                    for k, j in enumerate(damaged):  # a bit of a primary chunk inside the first frame of the first range
                        f0 = int(start[j * per]) // FRAME
                        x = shift + int(frame_off[j * caps + f0]) + 2000
                        at.append(off[j] + RB.chunk_off(x // C * spc + x % C // 1024, 8 * spc) + 17 * k % 1024)
                    at = torch.tensor(at, dtype=torch.int64, device="cuda")
                    buf[at] ^= 0x10

                    # the host-planned call: arrays converted once, no wrapper in between
                    coff, clen, ctotal, nseg, stage, vseg = layout(L, fmt, n_cl, n_pad, frame_off, idx_off, nframes, plain,
                                                                   rs, start, rlen)
                    h_content = torch.zeros(ctotal + 16, dtype=torch.uint8, device="cuda")
                    h_status, h_used, h_vouch = (torch.zeros(nreq, dtype=torch.int32, device="cuda") for _ in range(3))
                    h_scratch = D.frame_read_scratch(nreq, nseg, stage, vseg, S)

                    def host():
                        rc = L.chipf_read_ranges_dev(fmt, pk, pv, None, ptr(frame_off), ptr(idx_off), ptr(nframes),
                                                     ptr(plain), vp(buf), ptr(n_off), ptr(n_len), vp(hashes), ptr(n_pad),
                                                     ptr(n_cl), S, ptr(rs), ptr(start), ptr(rlen), nreq, vp(h_content),
                                                     ptr(coff), ptr(clen), vp(h_status), vp(h_used), vp(h_vouch), 0,
                                                     vp(h_scratch), h_scratch.numel(), None)
                        assert rc == 0, rc

                    # the device-planned call: the requests as device tensors
                    d_rs, d_start, d_len = dev(rs, "int32"), dev(start, "int64"), dev(rlen, "int64")
                    content = torch.zeros(nreq * RANGE, dtype=torch.uint8, device="cuda")
                    d_clen = torch.zeros(nreq, dtype=torch.int64, device="cuda")
                    status, used, vouch = (torch.zeros(nreq, dtype=torch.int32, device="cuda") for _ in range(3))
                    scratch = D.planned_frame_read_scratch(table, ftab, nreq, RANGE)

                    def planned():
                        D.read_frame_ranges_planned(table, ftab, ktab, d_rs, d_start, d_len, RANGE, content, RANGE, d_clen,
                                                    status, used, vouch, scratch)

                    side = torch.cuda.Stream()
                    with torch.cuda.stream(side):
                        planned()
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=side):
                        planned()

                    # every request's bytes against the objects, the words against the host-planned call's
                    src = d_rs.to(torch.int64) * SEG + d_start
                    want = inp[src[:, None] + torch.arange(RANGE, device="cuda")[None, :]]
                    h_content.fill_(0x5A)
                    host()
                    torch.cuda.synchronize()
                    got = h_content[torch.from_numpy(coff.astype("int64")).cuda()[:, None] +
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

                    r = {"requests": nreq, "work_items": int(nseg), "damaged": len(damaged),
                         "scratch_bytes": scratch.numel(), "host_planned_scratch_bytes": h_scratch.numel(),
                         "staging_bytes": nreq * ((FCAP * int(ftab.max_frame) + 15) // 16 * 16),
                         "host_planned_staging_bytes": int(stage),
                         **time_forms({"planned": planned, "host": host, "replay": graph.replay}, args.reps)}
                    r["planned_over_host"] = round(r["planned"]["median_ms"] / r["host"]["median_ms"], 3)
                    r["replay_over_host"] = round(r["replay"]["median_ms"] / r["host"]["median_ms"], 3)
                    level[f"read_{per}_{name}"] = cells[fmt, corpus, per, name] = r
                    buf[at] ^= 0x10   # the streams as they were
                    torch.cuda.synchronize()
                    del content, h_content, scratch, h_scratch, graph, want, got
                    torch.cuda.empty_cache()
            if ktab is not None:
                D.wipe_key_table(ktab)
            torch.cuda.synchronize()
            del buf, table, ftab, ktab
            torch.cuda.empty_cache()
        del inp
        torch.cuda.empty_cache()

    res["clocks"] = clocks.stop()
    is_a = lambda k: k[1] == "random" and k[2] == 16  # noqa: E731
    res["a_random_16_planned_median_below_host_min"] = all(
        r["planned"]["median_ms"] < r["host"]["min_ms"] for k, r in cells.items() if is_a(k))
    res["b_elsewhere_planned_median_not_above_host_max"] = all(
        r["planned"]["median_ms"] <= r["host"]["max_ms"] for k, r in cells.items() if not is_a(k))
    res["b_cells_above_host_max"] = ["level%d_%s read_%d_%s" % k for k, r in cells.items()
                                     if not is_a(k) and r["planned"]["median_ms"] > r["host"]["max_ms"]]
    ratios = {}
    for (fmt, corpus, per, name), r in cells.items():
        if per == 16:
            one = cells[fmt, corpus, 1, name]
            ratios[f"level{fmt}_{corpus}_{name}"] = {
                "host_median_ms_1024": one["planned"]["host_median_ms"],
                "host_median_ms_16384": r["planned"]["host_median_ms"],
                "ratio": round(r["planned"]["host_median_ms"] / one["planned"]["host_median_ms"], 3),
                "host_planned_ratio": round(r["host"]["host_median_ms"] / one["host"]["host_median_ms"], 3)}
    res["c_planned_host_time"] = ratios
    res["c_planned_host_time_same_within_1p5x"] = all(v["ratio"] <= 1.5 for v in ratios.values())
    line = json.dumps(res)
    print(line)
    partial = args.corpus or args.level
    if args.out and not (partial and args.out == ap.get_default("out")):  # a partial run never replaces the profile
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
