"""Writes tests/golden/extreme_keys.json: keys whose moduli sit at the worst case of the
reduced-radix Montgomery engine's magnitude bounds (DESIGN.md "Extreme moduli"), where the
committed random keys (modulus limbs averaging 2^27) never get.  Plain Python, deterministic (no
random source: g and h come from SHA-256 in counter mode), not run by the tests.  Prints, for
every modulus a kernel reduces by, the number of its 28-bit limbs that equal 2^28 - 1 and
-N^-1 mod 2^28.

Paillier (key_bits k in 1024, 2048, 4096; real primes, the key holder reduces exponents mod
p(p-1)):
  ones      the two largest primes below 2^(k/2): n, n^2, p^2, q^2 are runs of all-ones limbs,
            and nearly every 4-bit window of n and p - 1 is 0xF
  ones_lo1  the two largest primes below 2^(k/2) that are 1 mod 2^32: every modulus is 1 mod
            2^32, so -N^-1 is all ones in the 28-bit engine radix and in the 32-bit host radix
  sparse    the two smallest primes above 3 2^(k/2-2): long zero runs in moduli and exponents
OU, public only (any odd n of the right length is accepted; b in 2048, 4096):
  allones   2^b - 1           every limb but the top all ones; R mod n is a small power of two
  ones_lo1  2^b - 2^32 + 1    all-ones limbs and -N^-1 all ones
  sparse    2^(b-1) + 1       two non-zero limbs
each with a fixed g, h in [2, n-2] coprime to n.
OU, real: p the largest prime below 2^683, q the largest below 2^682 (3 x 683 = 2049, so two
683-bit primes give bits(p^2 q) = 2049; this is the nearest pair with bits(p^2 q) = 2048), g the
first hash-derived value with g^(p-1) mod p^2 != 1.
"""
import hashlib
import json
import math
import os
import time

HERE = os.path.dirname(os.path.abspath(__file__))
LB = 28
MASK = (1 << LB) - 1


def _small_primes(bound):
    sieve = bytearray([1]) * bound
    sieve[:2] = b"\0\0"
    for i in range(2, int(bound ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = bytearray(len(sieve[i * i::i]))
    return [i for i in range(bound) if sieve[i]]


SMALL = _small_primes(20000)
MR_BASES = SMALL[:40]


def is_prime(n):
    """Trial division, then Miller-Rabin to the first 40 prime bases."""
    if n < 2:
        return False
    for s in SMALL:
        if n % s == 0:
            return n == s
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_from(start, step, count):
    """The first `count` primes of start, start + step, start + 2 step, ..."""
    out, c = [], start
    while len(out) < count:
        if is_prime(c):
            out.append(c)
        c += step
    return out


def hashed(label, n):
    """A value in [2, n-2] coprime to n, from SHA-256(label | counter) in counter mode."""
    ctr = 0
    while True:
        need, buf, i = (n.bit_length() + 7) // 8 + 8, b"", 0
        while len(buf) < need:
            buf += hashlib.sha256(f"{label}|{ctr}|{i}".encode()).digest()
            i += 1
        v = 2 + int.from_bytes(buf[:need], "big") % (n - 3)
        if math.gcd(v, n) == 1:
            return v
        ctr += 1


def paillier_pair(family, k):
    h = k // 2
    if family == "ones":
        p, q = sorted(primes_from((1 << h) - 1, -2, 2))
    elif family == "ones_lo1":
        p, q = sorted(primes_from((1 << h) - (1 << 32) + 1, -(1 << 32), 2))
        assert p % (1 << 32) == 1 and q % (1 << 32) == 1
    else:
        p, q = sorted(primes_from(3 * (1 << (h - 2)) + 1, 2, 2))
    assert (p * q).bit_length() == k and p != q
    assert (p - 1) % q != 0 and (q - 1) % p != 0  # the direct-z key-holder path stays on
    return p, q


def stats(name, N):
    limbs = [(N >> (LB * i)) & MASK for i in range((N.bit_length() + LB - 1) // LB)]
    return "%-28s %5d bits  %3d of %3d limbs all ones  %3d zero  -N^-1 mod 2^28 = 0x%07x" % (
        name, N.bit_length(), sum(1 for v in limbs if v == MASK), len(limbs), sum(1 for v in limbs if v == 0),
        (-pow(N, -1, 1 << LB)) & MASK)


def main():
    t0 = time.time()
    out = {"paillier": {}, "ou_public": {}, "ou_keys": {}}
    lines = []
    for k in (1024, 2048, 4096):
        for family in ("ones", "ones_lo1", "sparse"):
            p, q = paillier_pair(family, k)
            name = f"{family}_{k}"
            out["paillier"][name] = {"bits": k, "family": family, "p": format(p, "x"), "q": format(q, "x")}
            n = p * q
            for tag, N in (("n^2", n * n), ("n", n), ("p^2", p * p), ("q^2", q * q), ("p", p), ("q", q)):
                lines.append(stats(f"paillier {name} {tag}", N))
    for b in (2048, 4096):
        for family, n in (("allones", (1 << b) - 1), ("ones_lo1", (1 << b) - (1 << 32) + 1), ("sparse", (1 << (b - 1)) + 1)):
            assert n.bit_length() == b and n % 2 == 1
            name = f"{family}_{b}"
            out["ou_public"][name] = {"bits": b, "family": family, "n": format(n, "x"),
                                      "g": format(hashed(f"g|{name}", n), "x"), "h": format(hashed(f"h|{name}", n), "x")}
            lines.append(stats(f"ou_public {name} n", n))
    p = primes_from((1 << 683) - 1, -2, 1)[0]
    q = primes_from((1 << 682) - 1, -2, 1)[0]
    n = p * p * q
    assert n.bit_length() == 2048 and p != q
    ctr = 0
    while True:
        g = hashed(f"g|ou_ones_2048|{ctr}", n)
        if pow(g, p - 1, p * p) != 1:
            break
        ctr += 1
    out["ou_keys"]["ones_2048"] = {"bits": 2048, "family": "ones", "p": format(p, "x"), "q": format(q, "x"),
                                   "g": format(g, "x")}
    lines.append(stats("ou ones_2048 n", n))
    lines.append(stats("ou ones_2048 p^2", p * p))
    with open(os.path.join(HERE, "extreme_keys.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("\n".join(lines))
    print("generated in %.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
