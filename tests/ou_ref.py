"""Okamoto-Uchiyama in plain Python integers -- the oracle of the OU tests, written from the
scheme's formulas (rust/fate_utils/crates/ou/src/lib.rs:69-138; fixedpoint_ou/src/lib.rs):
n = p^2 q, h = g^n mod n, encrypt(m, r) = g^m h^r mod n, decrypt(c) = L(c^(p-1) mod p^2)
L(g^(p-1) mod p^2)^-1 mod p with L(x) = (x - 1) / p.  Ciphertexts are canonical residues mod n
(the reference leaves a fresh ciphertext's product unreduced)."""
import json
import os
from typing import Dict, List, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))


class Key:
    def __init__(self, p: int, q: int, g: int):
        self.p, self.q, self.g = p, q, g
        self.n = p * p * q
        self.h = pow(g, self.n, self.n)
        self.p2 = p * p
        self.hp = pow((pow(g, p - 1, self.p2) - 1) // p, -1, p)


def load_keys() -> Dict[int, Key]:
    with open(os.path.join(HERE, "golden", "ou_keys.json")) as f:
        fx = json.load(f)["keys"]
    return {int(b): Key(int(k["p"], 16), int(k["q"], 16), int(k["g"], 16)) for b, k in fx.items()}


def encrypt(k: Key, m: int, r: int) -> int:
    return pow(k.g, m, k.n) * pow(k.h, r, k.n) % k.n


def decrypt(k: Key, c: int) -> int:
    return (pow(c, k.p - 1, k.p2) - 1) // k.p * k.hp % k.p


def align(k: Key, c: int, gap: int) -> int:
    """decrese_exp_to: c^(16^gap) mod n."""
    return pow(c, 16 ** gap, k.n)


def add(k: Key, a: Tuple[int, int], b: Tuple[int, int]) -> Tuple[int, int]:
    """Ciphertext::add on (c, exp) pairs: the literal 1 is the identity (the other operand is
    returned as it is), else both are brought to the lower exponent and multiplied mod n."""
    (ca, ea), (cb, eb) = a, b
    if ca == 1:
        return cb, eb
    if cb == 1:
        return ca, ea
    if ea > eb:
        ca, ea = align(k, ca, ea - eb), eb
    elif eb > ea:
        cb, eb = align(k, cb, eb - ea), ea
    return ca * cb % k.n, ea


def neg(k: Key, c: int) -> int:
    return pow(c, -1, k.n)


def mul(k: Key, c: int, pt: int) -> int:
    return pow(c, pt, k.n)


def pack_floats(xs: List[float], offset_bit: int, pack_num: int, precision: int) -> List[int]:
    """fixedpoint_ou/src/lib.rs:69-84: per chunk, x = (x << offset_bit) + round(v 2^precision)
    (MPFR round: half away from zero; exact here, the products are computed in integers)."""
    from fractions import Fraction
    out = []
    for i in range(0, len(xs), pack_num):
        x = 0
        for v in xs[i:i + pack_num]:
            f = Fraction(v) * (1 << precision)
            r = (abs(f.numerator) * 2 + f.denominator) // (2 * f.denominator)
            x = (x << offset_bit) + (r if f >= 0 else -r)
        out.append(x)
    return out


def unpack_floats(packed: List[int], offset_bit: int, pack_num: int, precision: int, total: int) -> List[float]:
    """fixedpoint_ou/src/lib.rs:85-108."""
    from fractions import Fraction
    mask = (1 << offset_bit) - 1
    out = []
    for x in packed:
        n = min(total, pack_num)
        tmp = []
        for _ in range(n):
            tmp.append(float(Fraction(x & mask, 1 << precision)))
            x >>= offset_bit
        out.extend(reversed(tmp))
        total -= n
    return out
