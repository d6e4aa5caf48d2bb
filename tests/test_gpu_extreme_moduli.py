"""The Montgomery engine on worst-case moduli (DESIGN.md "Extreme moduli"; fixture tests/golden/
extreme_keys.json): all-ones limbs in the modulus, -N^-1 all ones, two-limb moduli, all-0xF and
long-zero exponents -- with operands whose resident form M(c) = c R mod N is itself at the edge
(tests/extreme_ref.py).  Every comparison is bit-exact against Python integers, oracle/
paillier_oracle.py, tests/ou_ref.py or libgmp (oracle/gmp_ref.py, where Python's pow at 8192 bits
would dominate the time).

(a) a public-only OU context accepts any odd n of the right length as its ciphertext modulus, so
    add, mul (c^pt mod n), align, pack_squeeze, the folds, neg, import / export and fphe_ou_encrypt
    are a general modular-arithmetic harness at TPI 2 (2048 bits) and TPI 4 (4096 bits);
(b) the real OU key of all-ones primes: encrypt and the full-width c^(p-1) mod p^2 of decrypt;
(c) Paillier keys of three families x {1024, 2048, 4096} bits through both kernels of each op
    (kernel_path): n^2 at TPI 2 / 4 / 8, p^2 and q^2 at TPI 1 / 2 / 4."""
import math
import random
from types import SimpleNamespace

import pytest
import torch

from fate_amd import ou
from fate_amd import paillier as P
from fate_amd.paillier import PlaintextVector
from oracle import gmp_ref
from oracle import paillier_oracle as O
from tests import extreme_ref as X
from tests import ou_ref
from tests.test_gpu_edges import run_extreme_operands

pytestmark = pytest.mark.gpu

FX = X.load_fixture()
OU_PUBLIC = sorted(FX["ou_public"])
PAILLIER = sorted(FX["paillier"])


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# --------------------------------------------------------------------------------------
# (a) modulus-only operations on the public OU contexts
# --------------------------------------------------------------------------------------
_ENV = {}


def _env(name):
    """(N, pk, operands, padded operand vector) of a public OU modulus, made once: fate_amd.ou
    registers a public key by its modulus, so one (g, h) serves the whole module."""
    if name not in _ENV:
        k = FX["ou_public"][name]
        N, g, h = int(k["n"], 16), int(k["g"], 16), int(k["h"], 16)
        pk = ou.PK(N, g, h)
        L2 = pk._key.L2
        assert L2 == (64 if k["bits"] <= 2048 else 128)
        R = X.mont_r(pk._key, _dev())
        assert R == (1 << (X.LB * X.LL * (L2 // 32))) % N  # the engine's R, as the context reports it
        res = X.resident_patterns(N, L2)
        ops = X.canonical(res, R, N) + [0, 1, 2, N - 1]
        if k["family"] == "allones":  # (2^(b/2) - 1)(2^(b/2) + 1) = n: the product is stored as 0, not n
            ops += [(1 << (k["bits"] // 2)) - 1, (1 << (k["bits"] // 2)) + 1]
        rng = random.Random(k["bits"] + len(name))
        count = 130 if L2 == 64 else 65  # ragged: two tiles and a bit, one and a bit
        padded = ops + [rng.randrange(N) for _ in range(count - len(ops))]
        _ENV[name] = SimpleNamespace(N=N, g=g, h=h, pk=pk, L2=L2, L1=L2 // 2, R=R, res=res, ops=ops, padded=padded,
                                     key=SimpleNamespace(n=N), bits=k["bits"], family=k["family"])
    return _ENV[name]


def _vec(e, cs, exps=None):
    return ou.CiphertextVector.from_signed_ints(cs, exps or [0] * len(cs), e.N, device="cuda")


def _ints(e, v):
    if v.n is None:
        v.n = e.N
    cs, es = v.to_signed_ints(e.N)
    assert not bool(v.sign[: v.count].any())
    return cs, es


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_resident_patterns_reach_the_device(name):
    """from_signed_ints -> to_signed_ints round trip, and the stored words of the pattern operands
    are the limb patterns themselves."""
    import numpy as np
    e = _env(name)
    v = _vec(e, e.padded, [i % 5 - 2 for i in range(len(e.padded))])
    assert _ints(e, v) == (e.padded, [i % 5 - 2 for i in range(len(e.padded))])
    rows = P.tiles_to_cols(v.C).t()[: len(e.res)].cpu().numpy().view(np.uint32)
    assert [sum(int(w) << (32 * k) for k, w in enumerate(r)) for r in rows] == e.res
    limbs = [[(x >> (28 * i)) & X.MASK for i in range(X.LL * e.L2 // 32)] for x in e.res]
    assert max(sum(1 for t in row if t == X.MASK) for row in limbs) >= (e.bits - 1) // 28 - 1


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_add_grid(name):
    """a b mod N over the operand x operand grid at equal exponents (zero products stored as 0)."""
    e = _env(name)
    m = len(e.ops)
    a = [e.ops[i // m] for i in range(m * m)] + [e.ops[0]]  # m^2 + 1: a ragged last tile
    b = [e.ops[i % m] for i in range(m * m)] + [e.ops[1]]
    got, exps = _ints(e, _vec(e, a).add(e.pk, _vec(e, b)))
    assert got == [x * y % e.N for x, y in zip(a, b)] and exps == [0] * len(a)
    assert 0 in got and e.N not in got
    if e.family == "allones":
        i = next(i for i in range(m * m) if (a[i], b[i]) == (e.ops[-2], e.ops[-1]))
        assert a[i] * b[i] == e.N and got[i] == 0


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_add_with_gaps(name):
    """a^(16^g) b mod N for exponent gaps 1, 2 and 31, on either side (Ciphertext::add's rule for
    the literal 1 included: tests/ou_ref.py)."""
    e = _env(name)
    a = e.padded
    b = a[7:] + a[:7]
    for gap in (1, 2, 31):
        ea = [gap if i % 2 == 0 else 0 for i in range(len(a))]
        eb = [0 if i % 2 == 0 else gap for i in range(len(a))]
        got = _ints(e, _vec(e, a, ea).add(e.pk, _vec(e, b, eb)))
        want = [ou_ref.add(e.key, (x, s), (y, t)) for x, s, y, t in zip(a, ea, b, eb)]
        assert got == ([w[0] for w in want], [w[1] for w in want]), gap


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_align(name):
    """c^(16^gap) mod N for gaps 0, 1, 5, 31 of every operand."""
    e = _env(name)
    gaps = (0, 1, 5, 31)
    cs = [c for c in e.ops for _ in gaps] + [e.padded[-1]]
    gs = [g for _ in e.ops for g in gaps] + [31]
    got, _ = _ints(e, P._align(e.pk, _vec(e, cs), torch.tensor(gs)))
    assert got == [pow(c, 16 ** g, e.N) for c, g in zip(cs, gs)]


def _plaintexts(L1):
    w = 32 * L1
    return [0, 1, 2, (1 << 28) - 1, 1 << 28, (1 << w) - 1, int("a" * (w // 4), 16), int("5" * (w // 4), 16), 1 << (w - 1)]


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_mul(name):
    """pow(c, pt, N) of every operand by every plaintext: 0, 1, 2, 2^28 - 1, 2^28, all ones over
    the L1 plaintext words, 0xAAAA.., 0x5555.., the single top bit (libgmp's mpz_powm)."""
    e = _env(name)
    pts = _plaintexts(e.L1)
    cs = [c for c in e.ops for _ in pts]
    ts = [t for _ in e.ops for t in pts]
    got, _ = _ints(e, _vec(e, cs).mul(e.pk, PlaintextVector.from_ints(ts, [0] * len(ts), device="cuda", lp=e.L1)))
    want = [gmp_ref.powm(c, t, e.N) if t > 2 else pow(c, t, e.N) for c, t in zip(cs, ts)]
    assert got == want
    assert want[:2] == [1, e.ops[0]] and pow(0, 0, e.N) == 1  # c^0 = 1, for c = 0 too (mpz_powm)


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_pack_squeeze_both_paths(name):
    """acc = acc^(2^offset) y mod N per chunk of 3, through fphe_pack_squeeze (one launch) and the
    stepwise fphe_sqmul path."""
    e = _env(name)
    off = 61
    want = []
    for i in range(0, len(e.padded), 3):
        acc = e.padded[i]
        for y in e.padded[i + 1:i + 3]:
            acc = pow(acc, 1 << off, e.N) * y % e.N
        want.append(acc)
    for wide in (1 << 20, 0):
        with P.path_options(wide_squeeze_max=wide):
            got = _ints(e, _vec(e, e.padded, [3] * len(e.padded)).pack_squeeze(3, off, e.pk))
        assert got == (want, [0] * len(want)), wide


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_neg(name):
    """pow(c, -1, N) of the operands that are units; every non-unit among them raises the
    reference's invert().unwrap() panic (as tests/test_gpu_ops.py::test_neg_not_invertible_panics)."""
    e = _env(name)
    us = [c for c in e.padded if math.gcd(c, e.N) == 1]
    bad = [c for c in e.ops if math.gcd(c, e.N) != 1]
    assert 0 in bad and len(us) > len(e.padded) // 4
    got, _ = _ints(e, _vec(e, us).neg(e.pk))
    assert got == [pow(c, -1, e.N) for c in us]
    for c in bad:
        with pytest.raises(P.PanicException):
            _vec(e, us[:5] + [c] + us[5:8]).neg(e.pk)


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_fold_segments(name):
    """Every operand folded into 3 segments, two exponents among the terms: the reference's
    sequential Ciphertext::add from the literal 1.  0 and the two factors of 2^b - 1 go to
    segment 2, which folds to 0; segments 0 and 1 are products of units and non-units."""
    e = _env(name)
    cs = e.padded
    zero_like = {0} | (set(e.ops[-2:]) if e.family == "allones" else set())
    seg = [2 if c in zero_like else i % 3 for i, c in enumerate(cs)]
    exps = [1 if i % 4 == 1 else 0 for i in range(len(cs))]
    out = P._fold_to_segments(e.pk, _vec(e, cs, exps), torch.tensor(seg), 3)
    want = [(1, 0)] * 3
    for c, s, x in zip(cs, seg, exps):
        want[s] = ou_ref.add(e.key, want[s], (c, x))
    assert _ints(e, out) == ([w[0] for w in want], [w[1] for w in want])
    assert want[2][0] == 0 and want[0][0] not in (0, 1) and want[1][0] not in (0, 1)


def _rs(n):
    bits = n.bit_length()
    return [1, 2, n - 1, (1 << (bits - 1)) - 1, 1 << (bits - 1)]


@pytest.mark.parametrize("name", OU_PUBLIC)
def test_ou_encrypt_fixed_base(name):
    """g^m h^r mod n from the fixed-base tables: r in {1, 2, n - 1, all ones below n, the single
    top bit} x m in {0, 1, all ones over the L1 plaintext words}."""
    e = _env(name)
    ms = [0, 1, (1 << (32 * e.L1)) - 1]
    pairs = [(m, r) for r in _rs(e.N) for m in ms]
    pv = PlaintextVector.from_ints([m for m, _ in pairs], [0] * len(pairs), device="cuda", lp=e.L1)
    got, _ = _ints(e, e.pk.encrypt_encoded(pv, True, r=[r for _, r in pairs]))
    assert got == [gmp_ref.powm(e.g, m, e.N) * gmp_ref.powm(e.h, r, e.N) % e.N for m, r in pairs]


# --------------------------------------------------------------------------------------
# (b) the real OU key of all-ones primes
# --------------------------------------------------------------------------------------
def test_ou_ones_key_encrypt_decrypt():
    """p, q the largest primes below 2^683, 2^682: n, p^2 and the exponent p - 1 are runs of ones.
    encrypt with the edge r against tests/ou_ref.py, and decrypt -- c^(p-1) mod p^2 on the full-
    width engine -- of those ciphertexts, of 1 and g, and of their products."""
    k = FX["ou_keys"]["ones_2048"]
    key = ou_ref.Key(int(k["p"], 16), int(k["q"], 16), int(k["g"], 16))
    assert key.n.bit_length() == 2048 and (key.p - 1) >> 16 == (1 << 667) - 1  # all 0xF windows but the low few
    sk, pk, coder = ou.keypair_from_primes(key.p, key.q, key.g)
    ms = [0, 1, key.p - 1, (1 << 682) - 1, (1 << 64) - 1]
    pairs = [(m, r) for r in _rs(key.n) for m in ms]
    pv = PlaintextVector.from_ints([m for m, _ in pairs], [0] * len(pairs), device="cuda", lp=pk._key.L1)
    ct = pk.encrypt_encoded(pv, True, r=[r for _, r in pairs])
    got, _ = ct.to_signed_ints(pk.ns)
    want = [ou_ref.encrypt(key, m, r) for m, r in pairs]
    assert got == want
    assert sk.decrypt_to_encoded(ct).to_ints()[0] == [m for m, _ in pairs] == [ou_ref.decrypt(key, c) for c in want]
    cs = [1, key.g] + [a * b % key.n for a, b in zip(want, want[1:])]
    dv = ou.CiphertextVector.from_signed_ints(cs, [0] * len(cs), key.n, device="cuda")
    sums = [0, 1] + [(a[0] + b[0]) % key.p for a, b in zip(pairs, pairs[1:])]
    assert sk.decrypt_to_encoded(dv).to_ints()[0] == sums == [ou_ref.decrypt(key, c) for c in cs]


# --------------------------------------------------------------------------------------
# (c) Paillier: three families x {1024, 2048, 4096}
# --------------------------------------------------------------------------------------
_PAI = {}


def _paillier(name):
    """Keys, inputs and the reference's results for one Paillier key, computed once (libgmp) and
    shared by both kernel paths.  35 (significand, r) pairs; 10 at 4096 bits, each significand
    and each r still present."""
    if name not in _PAI:
        k = FX["paillier"][name]
        p, q = int(k["p"], 16), int(k["q"], 16)
        n = p * q
        ns = n * n
        assert n.bit_length() == k["bits"]
        sigs = [0, 1, -1, n // 2, -(n // 2), n // 4, n // 4 + 1]
        rs = [1, 2, n - 1, n - 2, (1 << (k["bits"] - 1)) - 1]
        if k["bits"] <= 2048:
            pairs = [(s, r) for s in sigs for r in rs]
        else:
            pairs = [(sigs[i % 7], rs[i % 5]) for i in range(10)]
        gk = gmp_ref.GmpKey(n, p, q)
        enc = [gk.encrypt(s, r, True) for s, r in pairs]
        osk, opk = O.keypair_from_primes(p, q)
        assert enc[:2] == [O.encrypt(opk, s, True, r) for s, r in pairs[:2]]  # libgmp against the Python oracle
        _PAI[name] = SimpleNamespace(p=p, q=q, n=n, ns=ns, bits=k["bits"], pairs=pairs, enc=enc, gk=gk, osk=osk, opk=opk,
                                     crafted=None)
    return _PAI[name]


@pytest.mark.parametrize("name", PAILLIER)
def test_paillier_encrypt_decrypt(name, kernel_path):
    """Public and key-holder (CRT) encrypt with injected r in {1, 2, n - 1, n - 2, all ones below
    n} of significands {0, +-1, +-floor(n/2), floor(n/4), floor(n/4) + 1}; decrypt of those
    ciphertexts; decrypt of crafted ciphertexts whose resident form mod n^2 is an edge pattern."""
    t = _paillier(name)
    sk, pk, coder = P.keypair_from_primes(t.p, t.q)
    pub = P.keypair_from_primes(t.p, t.q, keyholder=False)[1]
    assert pk.keyholder and not pub.keyholder
    assert P.path_option(_dev(), pk._priv, "kh_direct_z") == 1
    sigs = [s for s, _ in t.pairs]
    rs = [r for _, r in t.pairs]
    pv = PlaintextVector.from_ints(sigs, [0] * len(sigs), device="cuda")
    want = (t.enc, [0] * len(sigs))
    c_pub = pub.encrypt_encoded(pv, True, r=rs)
    assert c_pub.to_signed_ints(pk.ns) == want
    c_kh = pk.encrypt_encoded(pv, True, r=rs)
    assert c_kh.to_signed_ints(pk.ns) == want
    plain = [s % t.n for s in sigs]
    assert sk.decrypt_to_encoded(c_kh).to_ints()[0] == plain
    assert sk.decrypt_to_encoded(c_pub).to_ints()[0] == plain
    if t.crafted is None:
        res = X.resident_patterns(t.ns, pk._key.L2)
        cs = X.units(X.canonical(res, X.mont_r(pk._key, _dev()), t.ns), t.ns)
        assert len(cs) == len(res)
        t.crafted = (cs, [t.gk.decrypt(c) for c in cs])
        assert t.crafted[1][:2] == [O.decrypt(t.osk, c) for c in cs[:2]]  # libgmp against the Python oracle
    cs, dec = t.crafted
    dv = P.CiphertextVector.from_signed_ints(cs, [0] * len(cs), pk.ns, pk._key.L2)
    assert sk.decrypt_to_encoded(dv).to_ints()[0] == dec


@pytest.mark.parametrize("bits", [1024, 2048, 4096])
def test_extreme_operands_on_ones_keys(bits, monkeypatch):
    """tests/test_gpu_edges.py::test_extreme_operands on the key whose n^2, p^2 and q^2 are
    themselves runs of all-ones limbs: edge operands against an edge modulus (12 operands at
    4096 bits, where the reference is the slow side; the oracle's powm is libgmp's mpz_powm,
    the call it restates, tests/test_oracle.py)."""
    monkeypatch.setattr(O, "powm", gmp_ref.powm)
    k = FX["paillier"][f"ones_{bits}"]
    run_extreme_operands(int(k["p"], 16), int(k["q"], 16), count=12 if bits > 2048 else None)


@pytest.mark.parametrize("name", PAILLIER)
def test_device_drawn_r_round_trip(name):
    """decrypt(encrypt(x)) == x with r (public key) and (z_p, z_q) (key holder) drawn on the
    device: for n just below a power of two the rejection sampler (chacha_dev.h) almost never
    rejects, for the sparse n = 0.5625 2^k it rejects a large share of its draws."""
    k = FX["paillier"][name]
    p, q = int(k["p"], 16), int(k["q"], 16)
    sk, pk, coder = P.keypair_from_primes(p, q)
    pub = P.keypair_from_primes(p, q, keyholder=False)[1]
    n = p * q
    sigs = [0, 1, -1, n // 2, -(n // 2), n // 4, n // 4 + 1] + list(range(2, 60))
    pv = PlaintextVector.from_ints(sigs, [0] * len(sigs), device="cuda")
    for key in (pk, pub):
        a, b = key.encrypt_encoded(pv, True), key.encrypt_encoded(pv, True)
        assert sk.decrypt_to_encoded(a).to_ints()[0] == [s % n for s in sigs]
        ca, cb = a.to_signed_ints(pk.ns)[0], b.to_signed_ints(pk.ns)[0]
        assert all(x != y for x, y in zip(ca, cb)) and len(set(ca)) == len(ca)
