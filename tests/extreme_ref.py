"""Operands for the GPU tests of the Montgomery engine's magnitude bounds (DESIGN.md "Extreme
moduli").  The kernels work on the resident value M(c) = c R mod N, so a canonical value such as
N - 1 reaches them as a random-looking limb pattern; these helpers go the other way: they list
resident limb patterns v at the bounds' edges and return the canonical c = v R^-1 mod N that is
stored as v.  R is read from the context (fphe_ctx_mont_one), never assumed."""
import json
import math
import os
from typing import List

HERE = os.path.dirname(os.path.abspath(__file__))
LB = 28  # fate_amd/csrc/radix.h: 28-bit limbs,
LL = 37  # 37 per lane, L2 / 32 lanes per element
MASK = (1 << LB) - 1


def load_fixture() -> dict:
    with open(os.path.join(HERE, "golden", "extreme_keys.json")) as f:
        return json.load(f)


def mont_r(key, device) -> int:
    """R mod N of a key context: the stored words of the literal 1."""
    import numpy as np
    w = key.mont_one(device).cpu().numpy().view(np.uint32)
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def resident_patterns(N: int, L2: int) -> List[int]:
    """Resident values v < N at the edges of the engine's bounds for a modulus of L2 words
    (NL = 37 L2 / 32 limbs, lane q holding limbs [37 q, 37 q + 37)):
    N - 1, N - 2, (N -+ 1) / 2; 2^(28 k) - 1 for the largest k that stays below N; every limb all
    ones (the top one as large as N allows) except limb j zero, j in {0, LL - 1, LL, NL - 1} -- the
    lane seams the DPP exchange and sweep() cross (a j above N's top limb names that top limb);
    alternating all-ones / zero limbs."""
    NL = LL * (L2 // 32)
    k = (N.bit_length() - 1) // LB
    while (1 << (LB * k)) - 1 >= N:
        k -= 1
    top = (N >> (LB * k)) - 1  # limb k of the largest all-ones value below N
    full = ((1 << (LB * k)) - 1) | (max(top, 0) << (LB * k))
    used = k + 1 if top > 0 else k
    out = [N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, (1 << (LB * k)) - 1]
    for j in (0, LL - 1, LL, NL - 1):
        j = min(j, used - 1)
        out.append(full & ~(MASK << (LB * j)))
    out.append(sum(MASK << (LB * i) for i in range(0, k, 2)))
    assert all(0 <= v < N for v in out)
    return list(dict.fromkeys(out))


def canonical(vs: List[int], R: int, N: int) -> List[int]:
    """c with c R mod N == v for each resident value v"""
    rinv = pow(R, -1, N)
    return [v * rinv % N for v in vs]


def units(cs: List[int], N: int) -> List[int]:
    return [c for c in cs if math.gcd(c, N) == 1]
