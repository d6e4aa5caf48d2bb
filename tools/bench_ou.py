#!/usr/bin/env python
"""Okamoto-Uchiyama rates on one device, one JSON line (stand-alone: bench.py is the Paillier
yardstick and stays as it is).

Times 2048-bit OU at --count elements (default 2^20): encrypt with device-drawn r, decrypt,
ct-add; and in the same process, as the yardstick, this backend's 1024-bit Paillier encrypt
and ct-add -- the same 2048-bit modulus width and the same engine instantiation, so their
Montgomery products per second are what the OU kernels should approach.  Every leg is
bracketed by fphe_clock_stamp (the shader clock it ran at, as bench.py reports it) and timed
with device events; the figure is the median of --repeats runs after --warmup.

Products per element come from the kernels' own arithmetic: the fixed-base windows a wave
executes (k_ou_encrypt27: every window of r, since some lane's digit is non-zero, minus the
first which is a load, plus the plaintext's windows), the sliding-window schedule of powm27
over the shared exponent (p - 1, or n for Paillier) plus its table build and conversions.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fate_amd import _lib, ou  # noqa: E402
from fate_amd import paillier as P  # noqa: E402

OU_WIN, SLIDE_WIN = 4, 6


def sliding_products(e: int, w: int) -> int:
    """powm27's products for exponent e: table (X^2 and 2^(w-1) - 1 odd powers), then per
    window its squarings and one product."""
    n = 1 + (1 << (w - 1)) - 1
    i = e.bit_length() - 1
    first = True
    while i >= 0:
        if not (e >> i) & 1:
            n += 1
            i -= 1
            continue
        j = max(i - w + 1, 0)
        while not (e >> j) & 1:
            j += 1
        n += 0 if first else (i - j + 1) + 1
        first = False
        i = j - 1
    return n


def stamp(dev, blocks=2048):
    out = torch.zeros(3 * blocks, dtype=torch.int64, device=dev)
    khz = ctypes.c_uint32()
    _lib.check(_lib.load().fphe_clock_stamp(P._ptr(out), blocks, ctypes.byref(khz),
                                            ctypes.c_void_p(P._stream(dev))), "fphe_clock_stamp")
    return out, khz.value


def leg_clock(s0, s1, khz):
    a, b = s0.cpu().view(-1, 3), s1.cpu().view(-1, 3)
    first = {int(r[0]): (int(r[1]), int(r[2])) for r in a.tolist()}
    mhz = []
    for cu, c1, w1 in b.tolist():
        if cu in first and w1 > first[cu][1]:
            mhz.append((c1 - first[cu][0]) / (w1 - first[cu][1]) * khz / 1e3)
    return round(statistics.median(mhz), 1) if mhz else None


def timed(dev, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms, clocks = [], []
    for _ in range(repeats):
        s0, khz = stamp(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        s1, _ = stamp(dev)
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
        clocks.append(leg_clock(s0, s1, khz))
    return statistics.median(ms), [c for c in clocks if c]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = a.count
    osk, opk, ocoder = ou.keygen(2048)
    psk, kpk, pcoder = P.keygen(1024)
    ppk = P.PK(kpk.n)  # public-only: the modexp r^n mod n^2 itself, not the key holder's CRT halves
    g = torch.Generator().manual_seed(1)
    vals = torch.randint(0, 2 ** 62, (n,), generator=g, dtype=torch.int64)
    opv = P.PlaintextVector.from_ints(vals.tolist(), [0] * n, device=dev, lp=2)
    ppv = pcoder.encode_f64_vec(torch.rand(n, generator=g, dtype=torch.float64).to(dev))
    legs = {}
    with P.path_options(**P.THROUGHPUT_PATHS):
        oct_ = opk.encrypt_encoded(opv, True)
        pct = ppk.encrypt_encoded(ppv, True)
        hwin = (2048 + OU_WIN - 1) // OU_WIN
        runs = [
            ("ou_encrypt", lambda: opk.encrypt_encoded(opv, True), hwin - 1 + (62 + OU_WIN - 1) // OU_WIN),
            ("ou_decrypt", lambda: osk.decrypt_to_encoded(oct_), 2 + sliding_products(osk.p - 1, SLIDE_WIN)),
            ("ou_add", lambda: oct_.add(opk, oct_), 1),
            ("paillier1024_encrypt", lambda: ppk.encrypt_encoded(ppv, True), 3 + sliding_products(ppk.n, SLIDE_WIN)),
            ("paillier1024_add", lambda: pct.add(ppk, pct), 1),
        ]
        for name, fn, prods in runs:
            ms, clocks = timed(dev, fn, a.warmup, a.repeats)
            legs[name] = {"ms": round(ms, 3), "elems_per_s": round(n / ms * 1e3), "products_per_elem": prods,
                          "products_per_s": round(n * prods / ms * 1e3),
                          "sclk_mhz": round(statistics.median(clocks), 1) if clocks else None}
    for name, yard in (("ou_encrypt", "paillier1024_encrypt"), ("ou_decrypt", "paillier1024_encrypt"),
                       ("ou_add", "paillier1024_add")):
        legs[name]["ratio_to_yardstick"] = round(legs[name]["products_per_s"] / legs[yard]["products_per_s"], 3)
    print(json.dumps({"bench": "ou", "device": torch.cuda.get_device_name(dev), "count": n, "key_bits": 2048,
                      "ou_window": OU_WIN, "warmup": a.warmup, "repeats": a.repeats, "legs": legs}))


if __name__ == "__main__":
    main()
