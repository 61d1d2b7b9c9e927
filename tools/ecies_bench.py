#!/usr/bin/env python3
"""Ecies on device-resident objects: the AES-256-GCM kernels of
include/carbonado_hip_ecies.h against the only way there was, the host round
trip (GPU only; not bench.py).

Sets: --count1 x 1 MiB, --count16 x 16 MiB, and the 256 tails of the archive
tools/ragged_bench.py uses (seed 1: file lengths uniform in [1 MiB, 16 MiB],
the remainder of each modulo 1 MiB).

Forms, every one over objects that start and end in HBM:
  raw_seal / raw_open    chipe_gcm_seal_ragged_dev / chipe_gcm_open_ragged_dev
                         with the caller's keys: the kernels alone
  env_seal / env_open    chipe_seal_ragged_dev / chipe_open_ragged_dev: with
                         the per-object key agreement on the host (host_ms)
  level12_enc / _dec     chipx_encode_ragged_dev / chipx_decode_ragged_dev at 12
                         over the plaintext: what K13 / KR cost without Ecies
  dev13_enc / dev13_dec  level 13 kept in HBM, one call each:
                         chipe_encode_ragged_dev / chipe_decode_ragged_dev at 13
                         (the envelope seal into the scratch, then the level-12
                         encode over the envelopes; the reverse for decode)
  host13_enc / _dec      the round trip: D2H of the plaintext into pinned
                         memory, chip_encode_host_batch at 13, H2D of the
                         streams; the reverse with chip_decode_host_batch
                         (uniform sets only: that call takes one n)

Before anything is timed every form's bytes are compared: seal against open,
the envelopes against chip_ecies_decrypt on the host, dev13 against host13
through each other's decode.  A time is between two HIP events around the
form; host_ms is the host clock around the same calls (for env_seal that is
the key agreement of every object, which dominates small objects).  3
warm-ups, the forms alternating within a round for --reps rounds; median (min -
max) in ms, GiB/s of plaintext, the GPU's clocks sampled meanwhile.  Prints
one JSON line (and writes it to --out).  --dry-run: the sets, their scratch
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

SEG = 1 << 20
SECRET = bytes(range(1, 33))
LAUNCHES = {"raw_seal": 3, "raw_open": 4, "env_seal": 4, "env_open": 5}  # dev13: these plus the level-12 call's


def up(x, a=16):
    return (x + a - 1) // a * a


def tails(seed=1, files=256):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1 << 20, (16 << 20) + 1, files)
    return [int(x) % SEG for x in lengths if int(x) % SEG]


def sets(args):
    return {"1MiB": [SEG] * args.count1, "16MiB": [16 * SEG - 97] * args.count16, "tails": tails()}


def describe(name, lens):
    L = _lib.lib()
    arr = (ctypes.c_uint64 * len(lens))(*lens)
    return {"objects": len(lens), "plain_bytes": int(sum(lens)), "items": int(sum(((n + 15) // 16 + 511) // 512 for n in lens)),
            "scratch_bytes": int(L.chipe_gcm_scratch_len(arr, len(lens))), "launches": LAUNCHES}


class Set:
    def __init__(self, lens, seed):
        import torch
        from carbonado_amd import device as D
        self.D, self.torch = D, torch
        self.lens, self.count = lens, len(lens)
        self.total = sum(lens)
        rng = np.random.default_rng(seed)
        self.keys = rng.integers(0, 256, 32 * self.count, dtype=np.uint8).tobytes()
        self.ivs = rng.integers(0, 256, 16 * self.count, dtype=np.uint8).tobytes()
        pub = (ctypes.c_uint8 * 65)()
        assert _lib.lib().chip_ecies_public_key(SECRET, pub) == 0
        self.pub = bytes(pub)
        # plaintexts, ciphertexts (at 1 mod 16, where an envelope puts them) and envelopes, 16-B aligned rows
        self.in_off, self.ct_off, self.env_off = [], [], []
        ip = cp = ep = 0
        for n in lens:
            self.in_off.append(ip)
            self.ct_off.append(cp + 1)
            self.env_off.append(ep)
            ip += up(n)
            cp += up(n + 1)
            ep += up(n + 97)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.plain = torch.randint(0, 256, (max(ip, 16),), dtype=torch.uint8, device="cuda", generator=g)
        self.back = torch.zeros_like(self.plain)
        self.ct = torch.zeros(max(cp, 16), dtype=torch.uint8, device="cuda")
        self.env = torch.zeros(max(ep, 16), dtype=torch.uint8, device="cuda")
        self.tags = torch.zeros(16 * self.count, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(self.count, dtype=torch.int32, device="cuda")
        self.scratch = D.gcm_scratch(lens)
        self.env_len = [n + 97 for n in lens]
        # level 12 over the plaintext and over the envelopes
        self.o12, self.l12, t12 = D.ragged_layout(12, lens, 256)
        self.o13, self.l13, t13 = D.ragged_layout(12, self.env_len, 256)
        self.s12 = torch.zeros(t12, dtype=torch.uint8, device="cuda")
        self.s13 = torch.zeros(t13, dtype=torch.uint8, device="cuda")
        self.h12 = torch.zeros((self.count, 32), dtype=torch.uint8, device="cuda")
        self.h13 = torch.zeros((self.count, 32), dtype=torch.uint8, device="cuda")
        self.rs12 = D.ragged_scratch(12, lens)
        self.rd12 = D.ragged_scratch(12, self.l12, decode=True)
        self.es13 = D.ecies_ragged_scratch(13, lens)
        self.ds13 = D.ecies_ragged_scratch(13, self.l13, decode=True)
        self.pad12 = self.pad13 = None
        self.uniform = len(set(lens)) == 1
        if self.uniform:
            n = lens[0]
            self.hstride = up(_lib.lib().chip_encode_max_len(n), 256)
            self.hin = torch.empty((self.count, up(n)), dtype=torch.uint8).pin_memory()
            self.hout = torch.empty((self.count, self.hstride), dtype=torch.uint8).pin_memory()
            self.hback = torch.empty((self.count, up(n)), dtype=torch.uint8).pin_memory()
            self.dstreams = torch.zeros((self.count, self.hstride), dtype=torch.uint8, device="cuda")
            self.hhash = np.zeros(32 * self.count, dtype=np.uint8)
            self.hlen = np.zeros(self.count, dtype=np.uint64)
            self.hinfo = (_lib.EncodeInfoC * self.count)()

    # ---- forms
    def raw_seal(self):
        self.D.gcm_seal_ragged(self.keys, self.ivs, self.plain, self.in_off, self.lens, self.ct, self.ct_off, self.tags,
                               self.scratch)

    def raw_open(self):
        self.D.gcm_open_ragged(self.keys, self.ivs, self.ct, self.ct_off, self.lens, self.tags, self.back, self.in_off,
                               self.status, self.scratch)

    def env_seal(self):
        self.D.ecies_seal_ragged(self.pub, self.plain, self.in_off, self.lens, self.env, self.env_off, self.scratch)

    def env_open(self, src=None):
        self.D.ecies_open_ragged(SECRET, self.env if src is None else src, self.env_off, self.env_len, self.back,
                                 self.in_off, self.status, self.scratch)

    def level12_enc(self):
        _, info = self.D.encode_ragged(12, self.plain, self.in_off, self.lens, self.s12, self.o12, self.h12, self.rs12)
        self.pad12 = [i.padding_len for i in info]

    def level12_dec(self):
        self.D.decode_ragged(12, self.s12, self.o12, self.l12, self.h12, self.pad12, self.back, self.in_off, self.status,
                             self.rd12)

    def dev13_enc(self):
        _, info = self.D.encode_ragged_ecies(13, self.pub, self.plain, self.in_off, self.lens, self.s13, self.o13,
                                             self.h13, self.es13)
        self.pad13 = [i.padding_len for i in info]

    def dev13_dec(self):
        self.D.decode_ragged_ecies(13, SECRET, self.s13, self.o13, self.l13, self.h13, self.pad13, self.back, self.in_off,
                                   self.status, self.ds13)

    def host13_enc(self):
        L, n = _lib.lib(), self.lens[0]
        self.hin.copy_(self.plain.view(self.count, up(n)), non_blocking=True)
        self.torch.cuda.current_stream().synchronize()
        rc = L.chip_encode_host_batch(13, self.pub, 65, None, ctypes.c_void_p(self.hin.data_ptr()), n, self.count, up(n),
                                      ctypes.c_void_p(self.hout.data_ptr()), self.hstride,
                                      self.hlen.ctypes.data_as(_lib.c_u64p), ctypes.c_void_p(self.hhash.ctypes.data),
                                      self.hinfo, 0, 0, 0)
        assert rc == 0, rc
        self.dstreams.copy_(self.hout, non_blocking=True)

    def host13_dec(self):
        L, n = _lib.lib(), self.lens[0]
        self.hout.copy_(self.dstreams, non_blocking=True)
        self.torch.cuda.current_stream().synchronize()
        pads = (ctypes.c_uint32 * self.count)(*[self.hinfo[o].padding_len for o in range(self.count)])
        olen = (ctypes.c_uint64 * self.count)()
        st = (ctypes.c_int32 * self.count)()
        rc = L.chip_decode_host_batch(13, SECRET, 32, ctypes.c_void_p(self.hhash.ctypes.data),
                                      ctypes.c_void_p(self.hout.data_ptr()), self.hlen.ctypes.data_as(_lib.c_u64p),
                                      self.count, self.hstride, pads, ctypes.c_void_p(self.hback.data_ptr()), up(n), olen,
                                      st, 0, 0, 0)
        assert rc == 0 and list(olen) == self.lens, rc
        self.back.view(self.count, up(n)).copy_(self.hback, non_blocking=True)

    # ---- every form's bytes, before anything is timed
    def _back_is_plain(self, what):
        self.torch.cuda.synchronize()
        assert int(self.status.abs().sum()) == 0, what
        for o in range(0, self.count, max(1, self.count // 64)):
            a, n = self.in_off[o], self.lens[o]
            assert self.torch.equal(self.back[a:a + n], self.plain[a:a + n]), (what, o)
        self.back.zero_()

    def check(self):
        L = _lib.lib()
        self.raw_seal()
        self.raw_open()
        self._back_is_plain("raw")
        self.env_seal()
        self.torch.cuda.synchronize()
        for o in sorted({0, self.count // 2, self.count - 1}):  # the host's ecies opens what the device sealed
            e = self.env[self.env_off[o]:self.env_off[o] + self.env_len[o]].cpu().numpy()
            out = np.zeros(max(self.lens[o], 1), dtype=np.uint8)
            olen = ctypes.c_uint64()
            assert L.chip_ecies_decrypt(SECRET, 32, ctypes.c_void_p(e.ctypes.data), e.size,
                                        ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(olen)) == 0
            a = self.in_off[o]
            assert bytes(out[:olen.value]) == bytes(self.plain[a:a + self.lens[o]].cpu().numpy())
        self.env_open()
        self._back_is_plain("env")
        self.level12_enc()
        self.level12_dec()
        self._back_is_plain("level12")
        self.dev13_enc()
        self.dev13_dec()
        self._back_is_plain("dev13")
        if self.uniform:
            self.host13_enc()
            self.host13_dec()
            self._back_is_plain("host13")
            # the device opens the host's level-13 streams: same format, other keys and nonces
            self.torch.cuda.synchronize()
            n13 = int(self.hlen[0])
            assert n13 == self.l13[0]
            for o in range(self.count):
                self.s13[self.o13[o]:self.o13[o] + n13] = self.dstreams[o, :n13]
            self.h13.copy_(self.torch.from_numpy(self.hhash.reshape(self.count, 32)))
            self.pad13 = [self.hinfo[o].padding_len for o in range(self.count)]
            self.dev13_dec()
            self._back_is_plain("host13 streams through dev13_dec")
            self.dev13_enc()  # (and leave the device's own streams in place for the timed decode)

    def forms(self):
        f = {k: getattr(self, k) for k in ("raw_seal", "raw_open", "env_seal", "env_open", "level12_enc", "level12_dec",
                                           "dev13_enc", "dev13_dec")}
        if self.uniform:
            f["host13_enc"], f["host13_dec"] = self.host13_enc, self.host13_dec
        return f


def time_forms(torch, forms, reps, total):
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
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "host_median_ms": round(statistics.median(host[k]), 4),
                  "plain_GiB_s": round(total / (1 << 30) / (med / 1e3), 2) if med > 0 else None}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--count1", type=int, default=1024)
    ap.add_argument("--count16", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="", help="comma-separated set names")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ecies_bench_mi355x.json"))
    args = ap.parse_args()
    all_sets = sets(args)
    if args.only:
        all_sets = {k: v for k, v in all_sets.items() if k in args.only.split(",")}
    res = {"tool": "ecies_bench", "seed": args.seed, "reps": args.reps, "dry_run": bool(args.dry_run),
           "timing": "HIP events around each form, host_median_ms = host clock around the same calls; one box, one run",
           "sets": {k: describe(k, v) for k, v in all_sets.items()}}
    if args.dry_run:
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
        s = Set(lens, args.seed + i)
        s.check()
        r = res["sets"][name]
        r["forms"] = time_forms(torch, s.forms(), args.reps, s.total)
        f = r["forms"]
        r["encrypt_over_level12"] = round(f["dev13_enc"]["median_ms"] / f["level12_enc"]["median_ms"], 2)
        if s.uniform:
            r["host13_enc_over_dev13_enc"] = round(f["host13_enc"]["median_ms"] / f["dev13_enc"]["median_ms"], 2)
            r["host13_dec_over_dev13_dec"] = round(f["host13_dec"]["median_ms"] / f["dev13_dec"]["median_ms"], 2)
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
