#!/usr/bin/env python3
"""The Ecies key agreement on the device (include/carbonado_hip_agree.h)
against the host's stage pool (GPU only; not bench.py).

Sets, all at level 13 over objects that start and end in HBM:
  1024 x 1 MiB and 16384 x 64 KiB, the same envelopes for seal and open.

Cells, each chipy_ form beside the chipe_ form it replaces (the yardstick, in
the same run, alternating within a round):
  seal / open      chipy_seal_ragged_dev / chipy_open_ragged_dev against
                   chipe_seal_ragged_dev / chipe_open_ragged_dev
  encode / decode  chipy_encode_ragged_dev / chipy_decode_ragged_dev at 13
                   against chipe_encode_ragged_dev / chipe_decode_ragged_dev
  key_table        chipy_key_table_dev against chipc_stream_keys_dev followed by
                   chipk_key_table_dev over the set's resident level-13 streams
  keys             chipy_seal_keys_dev / chipy_open_keys_dev alone: the two
                   kernels, for the predictions of DESIGN.md
A time is between two HIP events around the call, to completion; host_ms is the
host clock around the same call.  3 warm-ups, --reps rounds (at least 15);
median, min and max in ms.  Before anything is timed the chipy_ envelopes are
opened by the chipe_ call and the other way round.

The conditions the feature is built on, each reported as held or not:
  (a) at 16384 objects every chipy_ median is below the yardstick's minimum
  (b) at 1024 the seal and the encode medians are below the chipe_ minimum
  (c) at 1024 the open, the decode and the key table are not above the
      yardstick's maximum
  (d) the host time of every chipy_ call is flat from 1024 to 16384 up to
      planning (the ratio is reported; the seal's includes its RNG)
Prints one JSON line (and writes it to --out).  --dry: the sets, their scratch
and launch counts without a device.
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from carbonado_amd import _lib  # noqa: E402

SECRET = bytes(range(1, 33))
SETS = {"1024x1MiB": (1024, 1 << 20), "16384x64KiB": (16384, 64 << 10)}
LAUNCHES = {"seal_keys": 1, "open_keys": 1, "seal": 5, "open": 6}  # encode / decode: these plus the level-12 call's
PAIRS = ("seal", "open", "encode", "decode", "key_table")


def up(x, a=16):
    return (x + a - 1) // a * a


def describe(count, n):
    L = _lib.lib()
    lens = (ctypes.c_uint64 * count)(*([n] * count))
    return {"objects": count, "object_bytes": n, "plain_bytes": count * n,
            "keys_scratch_bytes": int(L.chipy_keys_scratch_len(count)),
            "envelope_scratch_bytes": int(L.chipy_envelope_scratch_len(lens, count)),
            "gcm_scratch_bytes": int(L.chipe_gcm_scratch_len(lens, count)),
            "encode_scratch_bytes": int(L.chipy_encode_scratch_len(13, lens, count)),
            "uploads_per_call": {"seal": "public table, receiver table 96 KiB, 32 B per object of scalars",
                                 "open": "public table, 32 B"},
            "copies_back": 0, "waits": 0, "launches": LAUNCHES}


class Set:
    def __init__(self, count, n, seed):
        import torch
        from carbonado_amd import device as D
        self.D, self.torch = D, torch
        self.count, self.lens = count, [n] * count
        pub = (ctypes.c_uint8 * 65)()
        assert _lib.lib().chip_ecies_public_key(SECRET, pub) == 0
        self.pub = bytes(pub)
        self.in_off = [o * up(n) for o in range(count)]
        self.env_off = [o * up(n + 97) for o in range(count)]
        self.env_len = [n + 97] * count
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.plain = torch.randint(0, 256, (count * up(n),), dtype=torch.uint8, device="cuda", generator=g)
        self.back = torch.zeros_like(self.plain)
        self.env = torch.zeros(count * up(n + 97), dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(count, dtype=torch.int32, device="cuda")
        self.o13, self.l13, t13 = D.ragged_layout(12, self.env_len, 256)
        self.s13 = torch.zeros(t13, dtype=torch.uint8, device="cuda")
        self.h13 = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        self.scr = {"e": D.gcm_scratch(self.lens), "y": D.envelope_scratch(self.lens),
                    "e_enc": D.ecies_ragged_scratch(13, self.lens), "y_enc": D.ecies_ragged_scratch_dev_keys(13, self.lens),
                    "e_dec": D.ecies_ragged_scratch(13, self.l13, decode=True),
                    "y_dec": D.ecies_ragged_scratch_dev_keys(13, self.l13, decode=True), "keys": D.agree_scratch(count)}
        self.kpub = torch.zeros(count * 96, dtype=torch.uint8, device="cuda")
        self.kkeys = torch.zeros(count * 48, dtype=torch.uint8, device="cuda")
        self.pads = self.cls = self.table = None

    def forms(self):
        D, s = self.D, self

        def seal(y):
            f = D.ecies_seal_ragged_dev_keys if y else D.ecies_seal_ragged
            f(s.pub, s.plain, s.in_off, s.lens, s.env, s.env_off, s.scr["y" if y else "e"])

        def open_(y):
            f = D.ecies_open_ragged_dev_keys if y else D.ecies_open_ragged
            f(SECRET, s.env, s.env_off, s.env_len, s.back, s.in_off, s.status, s.scr["y" if y else "e"])

        def encode(y):
            f = D.encode_ragged_ecies_dev_keys if y else D.encode_ragged_ecies
            _, info = f(13, s.pub, s.plain, s.in_off, s.lens, s.s13, s.o13, s.h13, s.scr["y_enc" if y else "e_enc"])
            s.pads, s.cls = [i.padding_len for i in info], [i.chunk_len for i in info]

        def decode(y):
            f = D.decode_ragged_ecies_dev_keys if y else D.decode_ragged_ecies
            f(13, SECRET, s.s13, s.o13, s.l13, s.h13, s.pads, s.back, s.in_off, s.status, s.scr["y_dec" if y else "e_dec"])

        def key_table(y):
            if y:
                s.kt = D.key_table_from_streams(s.table, SECRET, s.scr["kt"])
            else:
                keys, ivs, kstat = D.stream_keys(SECRET, s.s13, s.o13, s.l13, s.h13, s.pads, s.cls, s.scr["sk"])
                s.kt = D.key_table(keys, ivs, kstat)

        out = {}
        for name, fn in (("seal", seal), ("open", open_), ("encode", encode), ("decode", decode),
                         ("key_table", key_table)):
            out["chipy_" + name] = lambda fn=fn: fn(True)
            out["chipe_" + name] = lambda fn=fn: fn(False)
        out["chipy_seal_keys"] = lambda: D.seal_keys(s.pub, s.count, s.kpub, 96, s.kkeys, 48, s.scr["keys"])
        out["chipy_open_keys"] = lambda: D.open_keys(SECRET, s.kpub, 96, s.count, s.kkeys, 48, s.status, s.scr["keys"])
        return out

    def _back_is_plain(self, what):
        self.torch.cuda.synchronize()
        assert int(self.status.abs().sum()) == 0, what
        assert self.torch.equal(self.back, self.plain), what
        self.back.zero_()

    def check(self):
        f = self.forms()
        for a, b in (("chipy_seal", "chipe_open"), ("chipe_seal", "chipy_open"), ("chipy_encode", "chipe_decode"),
                     ("chipe_encode", "chipy_decode"), ("chipy_seal", "chipy_open")):
            f[a]()
            f[b]()
            self._back_is_plain(a + " -> " + b)
        f["chipy_encode"]()  # the streams the timed decodes and key tables read
        self.torch.cuda.synchronize()
        self.table = self.D.stream_table(self.s13, self.o13, self.l13, self.h13, self.pads, self.cls)
        self.scr["sk"] = self.D.stream_keys_scratch(self.count)
        self.scr["kt"] = self.D._scratch(_lib.lib().chipy_key_table_scratch_len(ctypes.byref(self.table.info)))
        f["chipy_key_table"]()
        mine = self.kt.table.clone()
        f["chipe_key_table"]()
        self.torch.cuda.synchronize()
        assert self.torch.equal(mine, self.kt.table), "key tables differ"


def time_forms(torch, forms, reps):
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms, host = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            f()
            host[k].append((time.perf_counter() - t0) * 1e3)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "host_median_ms": round(statistics.median(host[k]), 4), "host_min_ms": round(min(host[k]), 4)}
            for k, v in ms.items()}


def conditions(small, large):
    below_min = lambda f, k: f["chipy_" + k]["median_ms"] < f["chipe_" + k]["min_ms"]  # noqa: E731
    not_above_max = lambda f, k: f["chipy_" + k]["median_ms"] <= f["chipe_" + k]["max_ms"]  # noqa: E731
    ratio = {k: round(large["chipy_" + k]["host_median_ms"] / max(small["chipy_" + k]["host_median_ms"], 1e-6), 2)
             for k in PAIRS}
    return {"a_16384_every_median_below_yardstick_min": {k: below_min(large, k) for k in PAIRS},
            "b_1024_seal_and_encode_below_chipe_min": {k: below_min(small, k) for k in ("seal", "encode")},
            "c_1024_open_decode_key_table_not_above_yardstick_max": {k: not_above_max(small, k)
                                                                     for k in ("open", "decode", "key_table")},
            "d_host_ms_16384_over_1024": ratio}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "agree_bench_mi355x.json"))
    args = ap.parse_args()
    res = {"tool": "agree_bench", "seed": args.seed, "reps": args.reps, "dry_run": bool(args.dry), "level": 13,
           "timing": "HIP events around each call to completion, host_*_ms = host clock around the same call; "
                     "one box, one run, yardsticks in the same run",
           "sets": {k: describe(*v) for k, v in SETS.items()}}
    if args.dry:
        print(json.dumps(res))
        return
    assert args.reps >= 15
    import torch
    from bench import ClockSampler
    rc = _lib.lib().chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res["box"] = {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}
    clocks = ClockSampler(0)
    clocks.start()
    for i, (name, (count, n)) in enumerate(SETS.items()):
        s = Set(count, n, args.seed + i)
        s.check()
        res["sets"][name]["forms"] = time_forms(torch, s.forms(), args.reps)
        del s
        torch.cuda.empty_cache()
    res["clocks"] = clocks.stop()
    res["conditions"] = conditions(res["sets"]["1024x1MiB"]["forms"], res["sets"]["16384x64KiB"]["forms"])
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
