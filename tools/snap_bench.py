#!/usr/bin/env python3
"""Snappy on device-resident objects: the kernels of
include/carbonado_hip_snap.h against the only way there was for the levels
with the Snappy bit, the host round trip (GPU only; not bench.py).

Sets: --count1 x 1 MiB and --count16 x (16 MiB less the frame and envelope
overhead, the largest object the one-call forms take), each on two corpora:
  mix40    random runs of 1..40 bytes alternating with repeats of earlier
           output (tests/snap_data.py): every chunk compressed, about 3:1
  random   random bytes: every chunk stored raw
(8 distinct 1 MiB objects / 2 distinct 16 MiB objects, repeated over the set:
a block's work does not depend on the other objects.)

Forms, every one over objects that start and end in HBM:
  raw_snap / raw_unsnap    chips_snap_ragged_dev / chips_unsnap_ragged_dev
  level12_enc / level13_enc  chipx_ / chipe_encode_ragged_dev over the same
                           plain bytes: what the call costs without Snappy
  dev14_enc / dev14_dec    chips_encode_ragged_dev / chips_decode_ragged_dev at 14
  dev15_enc / dev15_dec    the same at 15
  host14_enc / _dec, host15_enc / _dec
                           the round trip: D2H of the objects into pinned
                           memory, chip_encode_host_batch at that level, H2D of
                           the streams; the reverse with chip_decode_host_batch

Before anything is timed the bytes are compared: unsnap of snap, the device's
level-14 streams against the host's (equal, no randomness), every decode
against the objects.  A time is between two HIP events around the form;
host_median_ms is the host clock around the same calls.  2 warm-ups, the forms
alternating within a round for --reps rounds; median (min - max) in ms, GiB/s
of object bytes.  Prints one JSON line (and writes it to --out).  --dry: the
sets, their blocks, slots, scratch and launch counts without a device.
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
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from carbonado_amd import _lib  # noqa: E402

SEG = 1 << 20
BIG = (16 << 20) - 10 - 8 * 256 - 97
SECRET = bytes(range(1, 33))
LAUNCHES = {"raw_snap": 3, "raw_unsnap": 4}  # the one-call forms: these plus the ragged / Ecies call's


def up(x, a=16):
    return (x + a - 1) // a * a


def sets(args):
    return {"1MiB": [SEG] * args.count1, "16MiB": [BIG] * args.count16}


def describe(lens):
    L = _lib.lib()
    arr = (ctypes.c_uint64 * len(lens))(*lens)
    enc14 = (ctypes.c_uint64 * len(lens))()
    off, total = (ctypes.c_uint64 * len(lens))(), ctypes.c_uint64()
    assert L.chips_encode_layout(14, arr, len(lens), 256, 56, off, enc14, ctypes.byref(total)) == 0
    return {"objects": len(lens), "object_bytes": int(sum(lens)), "blocks": int(sum((n + 65535) // 65536 for n in lens)),
            "slots": int(sum((n + 65535) // 65536 + 1 for n in lens)),
            "snap_scratch_bytes": int(L.chips_snap_scratch_len(arr, len(lens))),
            "unsnap_scratch_bytes": int(L.chips_unsnap_scratch_len(arr, arr, len(lens))),
            "encode14_scratch_bytes": int(L.chips_encode_scratch_len(14, arr, len(lens))),
            "encode15_scratch_bytes": int(L.chips_encode_scratch_len(15, arr, len(lens))),
            "decode14_scratch_bytes": int(L.chips_decode_scratch_len(14, enc14, arr, len(lens))),
            "worst_case_stream_bytes_14": int(total.value), "launches": LAUNCHES}


class Set:
    def __init__(self, lens, corpus, seed):
        import torch
        import snap_data as SD
        from carbonado_amd import device as D
        self.D, self.torch = D, torch
        self.lens, self.count, n = lens, len(lens), lens[0]
        self.n, self.total = n, sum(lens)
        pub = (ctypes.c_uint8 * 65)()
        assert _lib.lib().chip_ecies_public_key(SECRET, pub) == 0
        self.pub = bytes(pub)
        distinct = 8 if n <= SEG else 2
        rng = np.random.default_rng(seed)
        rows = [np.frombuffer(SD.mix(n, 40, seed + i), dtype=np.uint8) if corpus == "mix40"
                else rng.integers(0, 256, n, dtype=np.uint8) for i in range(distinct)]
        self.pitch = up(n)
        host = torch.zeros((self.count, self.pitch), dtype=torch.uint8)
        for o in range(self.count):
            host[o, :n] = torch.from_numpy(rows[o % distinct].copy())
        self.plain = host.cuda().view(-1)
        self.in_off = [o * self.pitch for o in range(self.count)]
        self.back = torch.zeros_like(self.plain)
        z = lambda k, dt=torch.uint8: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
        # raw snap / unsnap
        self.frame_pitch = up(D.snap_max_len(n))
        self.frame_off = [o * self.frame_pitch for o in range(self.count)]
        self.frames, self.frame_len = z(self.count * self.frame_pitch), z(self.count, torch.int64)
        self.status, self.got = z(self.count, torch.int32), z(self.count, torch.int64)
        self.snap_scr = D.snap_scratch(lens)
        self.unsnap_scr = D.snap_scratch([self.frame_pitch] * self.count, lens)
        self.flens = None
        # level 12 / 13 over the plain bytes
        self.o12, self.l12, t12 = D.ragged_layout(12, lens, 256)
        self.o13, self.l13, t13 = D.ragged_layout(12, [x + 97 for x in lens], 256)
        self.s12, self.s13 = z(t12), z(t13)
        self.h12, self.h13 = z((self.count, 32)), z((self.count, 32))
        self.rs12, self.es13 = D.ragged_scratch(12, lens), D.ecies_ragged_scratch(13, lens)
        # levels 14 and 15 on the device
        self.dev = {}
        for fmt in (14, 15):
            off, cap, tot = D.snap_encode_layout(fmt, lens, 256)
            self.dev[fmt] = dict(off=off, cap=cap, out=z(tot), hash=z((self.count, 32)),
                                 enc=D.snap_ragged_scratch(fmt, lens), dec=D.snap_ragged_scratch(fmt, cap, lens),
                                 olen=None, pads=None)
        # the host round trip
        self.hstride = up(_lib.lib().chip_encode_max_len(n), 256)
        self.hin = torch.empty((self.count, self.pitch), dtype=torch.uint8).pin_memory()
        self.hout = torch.empty((self.count, self.hstride), dtype=torch.uint8).pin_memory()
        self.hback = torch.empty((self.count, self.pitch), dtype=torch.uint8).pin_memory()
        self.dstreams = z((self.count, self.hstride))
        self.hhash = {f: np.zeros(32 * self.count, dtype=np.uint8) for f in (14, 15)}
        self.hlen = {f: np.zeros(self.count, dtype=np.uint64) for f in (14, 15)}
        self.hinfo = {f: (_lib.EncodeInfoC * self.count)() for f in (14, 15)}

    # ---- forms
    def raw_snap(self):
        self.D.snap_ragged(self.plain, self.in_off, self.lens, self.frames, self.frame_off, self.frame_len, self.snap_scr)

    def raw_unsnap(self):
        self.D.unsnap_ragged(self.frames, self.frame_off, self.flens, self.back, self.in_off, self.lens, self.got,
                             self.status, self.unsnap_scr)

    def level12_enc(self):
        self.D.encode_ragged(12, self.plain, self.in_off, self.lens, self.s12, self.o12, self.h12, self.rs12)

    def level13_enc(self):
        self.D.encode_ragged_ecies(13, self.pub, self.plain, self.in_off, self.lens, self.s13, self.o13, self.h13, self.es13)

    def dev_enc(self, fmt):
        d = self.dev[fmt]
        d["olen"], info = self.D.encode_ragged_snap(fmt, self.plain, self.in_off, self.lens, d["out"], d["off"], d["hash"],
                                                    d["enc"], pubkey=self.pub if fmt & 1 else None)
        d["pads"] = [i.padding_len for i in info]

    def dev_dec(self, fmt):
        d = self.dev[fmt]
        self.D.decode_ragged_snap(fmt, d["out"], d["off"], d["olen"], d["hash"], d["pads"], self.back, self.in_off,
                                  self.lens, self.got, self.status, d["dec"], secret_key=SECRET if fmt & 1 else None)

    def host_enc(self, fmt):
        L = _lib.lib()
        self.hin.copy_(self.plain.view(self.count, self.pitch), non_blocking=True)
        self.torch.cuda.current_stream().synchronize()
        rc = L.chip_encode_host_batch(fmt, self.pub if fmt & 1 else None, 65 if fmt & 1 else 0, None,
                                      ctypes.c_void_p(self.hin.data_ptr()), self.n, self.count, self.pitch,
                                      ctypes.c_void_p(self.hout.data_ptr()), self.hstride,
                                      self.hlen[fmt].ctypes.data_as(_lib.c_u64p),
                                      ctypes.c_void_p(self.hhash[fmt].ctypes.data), self.hinfo[fmt], 0, 0, 0)
        assert rc == 0, rc
        self.dstreams.copy_(self.hout, non_blocking=True)

    def host_dec(self, fmt):
        L = _lib.lib()
        self.hout.copy_(self.dstreams, non_blocking=True)
        self.torch.cuda.current_stream().synchronize()
        pads = (ctypes.c_uint32 * self.count)(*[self.hinfo[fmt][o].padding_len for o in range(self.count)])
        olen = (ctypes.c_uint64 * self.count)()
        st = (ctypes.c_int32 * self.count)()
        rc = L.chip_decode_host_batch(fmt, SECRET if fmt & 1 else None, 32 if fmt & 1 else 0,
                                      ctypes.c_void_p(self.hhash[fmt].ctypes.data), ctypes.c_void_p(self.hout.data_ptr()),
                                      self.hlen[fmt].ctypes.data_as(_lib.c_u64p), self.count, self.hstride, pads,
                                      ctypes.c_void_p(self.hback.data_ptr()), self.pitch, olen, st, 0, 0, 0)
        assert rc == 0 and list(olen) == self.lens, rc
        self.back.view(self.count, self.pitch).copy_(self.hback, non_blocking=True)

    # ---- every form's bytes, before anything is timed
    def _back_is_plain(self, what):
        self.torch.cuda.synchronize()
        assert int(self.status.abs().sum()) == 0, what
        for o in range(0, self.count, max(1, self.count // 64)):
            a = self.in_off[o]
            assert self.torch.equal(self.back[a:a + self.n], self.plain[a:a + self.n]), (what, o)
        self.back.zero_()

    def check(self):
        self.raw_snap()
        self.torch.cuda.synchronize()
        self.flens = self.frame_len.cpu().tolist()
        self.raw_unsnap()
        self._back_is_plain("raw")
        assert self.got.cpu().tolist() == self.lens
        self.level12_enc()
        self.level13_enc()
        for fmt in (14, 15):
            self.dev_enc(fmt)
            self.dev_dec(fmt)
            self._back_is_plain(f"dev{fmt}")
            # the host decodes its own streams last, so the timed host decode has them in place
        self.host_enc(14)
        self.torch.cuda.synchronize()
        d = self.dev[14]
        assert [int(x) for x in self.hlen[14]] == d["olen"]
        for o in sorted({0, self.count // 2, self.count - 1}):   # the same bytes from both paths
            ln = d["olen"][o]
            assert self.torch.equal(d["out"][d["off"][o]:d["off"][o] + ln], self.dstreams[o, :ln]), o
        self.host_dec(14)
        self._back_is_plain("host14")

    def forms(self):
        f = {"raw_snap": self.raw_snap, "raw_unsnap": self.raw_unsnap, "level12_enc": self.level12_enc,
             "level13_enc": self.level13_enc}
        for fmt in (14, 15):   # a level's host encode leaves the streams its host decode reads
            f[f"dev{fmt}_enc"] = lambda fmt=fmt: self.dev_enc(fmt)
            f[f"dev{fmt}_dec"] = lambda fmt=fmt: self.dev_dec(fmt)
            f[f"host{fmt}_enc"] = lambda fmt=fmt: self.host_enc(fmt)
            f[f"host{fmt}_dec"] = lambda fmt=fmt: self.host_dec(fmt)
        return f


def time_forms(torch, forms, reps, total):
    for f in forms.values():
        for _ in range(2):
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
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "host_median_ms": round(statistics.median(host[k]), 4),
                  "object_GiB_s": round(total / (1 << 30) / (med / 1e3), 2) if med > 0 else None}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--count1", type=int, default=1024)
    ap.add_argument("--count16", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated set names")
    ap.add_argument("--corpora", default="mix40,random")
    ap.add_argument("--dry", "--dry-run", dest="dry", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "snap_bench_mi355x.json"))
    args = ap.parse_args()
    all_sets = sets(args)
    if args.only:
        all_sets = {k: v for k, v in all_sets.items() if k in args.only.split(",")}
    res = {"tool": "snap_bench", "seed": args.seed, "reps": args.reps, "dry_run": bool(args.dry),
           "timing": "HIP events around each form, host_median_ms = host clock around the same calls; one box, one run",
           "sets": {k: describe(v) for k, v in all_sets.items()}}
    if args.dry:
        print(json.dumps(res))
        return
    import torch
    from bench import ClockSampler
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res["box"] = {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}
    clocks = ClockSampler(0)
    clocks.start()
    for i, (name, lens) in enumerate(all_sets.items()):
        res["sets"][name]["corpora"] = {}
        for corpus in args.corpora.split(","):
            s = Set(lens, corpus, args.seed + 10 * i)
            s.check()
            r = {"forms": time_forms(torch, s.forms(), args.reps, s.total)}
            f = r["forms"]
            r["stream_bytes_14"] = int(sum(s.dev[14]["olen"]))
            r["frame_bytes"] = int(sum(s.flens))
            for fmt in (14, 15):
                r[f"host{fmt}_enc_over_dev{fmt}_enc"] = round(f[f"host{fmt}_enc"]["median_ms"] / f[f"dev{fmt}_enc"]["median_ms"], 2)
                r[f"host{fmt}_dec_over_dev{fmt}_dec"] = round(f[f"host{fmt}_dec"]["median_ms"] / f[f"dev{fmt}_dec"]["median_ms"], 2)
            res["sets"][name]["corpora"][corpus] = r
            print(f"[snap_bench] {name} {corpus} done", file=sys.stderr, flush=True)
            del s
            torch.cuda.empty_cache()
    res["clocks"] = clocks.stop()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
