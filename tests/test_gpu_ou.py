"""Okamoto-Uchiyama on the device (fate_amd.ou, fphe_ou_*), integer-exact against the plain-Python
oracle tests/ou_ref.py at the committed key sizes: 1024 (padded inside 64-word ciphertexts),
1540 (the issue's odd size: bits(n) is no multiple of 32, so r's top word is partial), 1542
(bits(n) = 2 mod 4 and bits(p) = 514 = 2 mod 4: the top 4-bit window of r is a partial, 2-bit
one -- the case of every key size = 2 mod 4), 2048 (fills 64 words) and 3072 (the 128-word
geometry).  67 elements: a whole wave tile plus a partial one at both lanes-per-element
settings; the inverse is also run through its batch route (4096 elements and up)."""
import ctypes
import json
import os
import random

import pytest
import torch

from fate_amd import _lib, ou, protocol_ou
from fate_amd import paillier as P
from fate_amd.paillier import PlaintextVector
from tests import ou_ref
from tests.chacha_ref import draw_below_host

pytestmark = pytest.mark.gpu

KEYS = ou_ref.load_keys()
BITS = sorted(KEYS)
COUNT = 67
W = 4  # kOuWin (fate_amd/csrc/key_blob.h)
RNG_KEY = [0x01234567, 0x89ABCDEF, 0xDEADBEEF, 0x0BADF00D, 0x13579BDF, 0x2468ACE0, 0xFEEDFACE, 0x31415926]
NONCE = (0x5EED << 40) ^ 0xC0FFEE


@pytest.fixture(scope="module")
def objs():
    return {b: ou.keypair_from_primes(k.p, k.q, k.g) for b, k in KEYS.items()}


def _plain(ms, exps=None, lp=None):
    return PlaintextVector.from_ints(ms, exps or [0] * len(ms), device="cuda", lp=lp)


def _ms_rs(k, seed):
    rng = random.Random(seed)
    bits = k.n.bit_length()
    ms = [0, 1, 2 ** 64 - 1, 2 ** (k.p.bit_length() - 1) - 1, k.p - 1]
    top = W * ((bits - 1) // W)  # first bit of r's top window (2 bits wide when bits = 2 mod 4)
    rs = [1, k.n - 1, 1 << (W * 37), 1 << (bits - 1), 1 << top, (k.n >> top) << top]
    ms += [rng.randrange(k.p) for _ in range(COUNT - len(ms))]
    rs += [1 + rng.randrange(k.n - 1) for _ in range(COUNT - len(rs))]
    rng.shuffle(rs)
    return ms, rs


def _encrypt(objs, bits, ms, rs, exps=None):
    sk, pk, coder = objs[bits]
    return pk.encrypt_encoded(_plain(ms, exps, lp=pk._key.L1), True, r=rs)


@pytest.mark.parametrize("bits", BITS)
def test_encrypt_parity(objs, bits):
    k = KEYS[bits]
    sk, pk, coder = objs[bits]
    assert pk._key.L2 == (64 if bits <= 2048 else 128)
    ms, rs = _ms_rs(k, bits)
    ct = _encrypt(objs, bits, ms, rs)
    got, exps = ct.to_signed_ints(pk.ns)
    assert got == [ou_ref.encrypt(k, m, r) for m, r in zip(ms, rs)]
    assert exps == [0] * COUNT and not bool(ct.sign.any())
    if bits > 2048:
        return
    # short plaintext rows (2 words) index the same table (the row walk is the same code at 128 words)
    ct2 = pk.encrypt_encoded(_plain([m & (2 ** 64 - 1) for m in ms]), False, r=rs)
    assert ct2.to_signed_ints(pk.ns)[0] == [ou_ref.encrypt(k, m & (2 ** 64 - 1), r) for m, r in zip(ms, rs)]


@pytest.mark.parametrize("bits", BITS)
def test_decrypt_parity(objs, bits):
    k = KEYS[bits]
    sk, pk, coder = objs[bits]
    ms, rs = _ms_rs(k, bits + 1)
    cs = [1, k.g % k.n] + [ou_ref.encrypt(k, m, r) for m, r in zip(ms, rs)][: COUNT - 2]
    want = [0, 1] + ms[: COUNT - 2]
    ct = ou.CiphertextVector.from_signed_ints(cs, [0] * COUNT, k.n, device="cuda")
    assert ct.L2 == pk._key.L2
    got, _ = sk.decrypt_to_encoded(ct).to_ints()
    assert got == want == [ou_ref.decrypt(k, c) for c in cs]
    # device encrypt -> device decrypt
    assert sk.decrypt_to_encoded(_encrypt(objs, bits, ms, rs)).to_ints()[0] == ms


@pytest.mark.parametrize("bits", [1540, 1542, 3072])
def test_device_drawn_r(objs, monkeypatch, bits):
    k = KEYS[bits]
    sk, pk, coder = objs[bits]
    monkeypatch.setattr(pk._key, "rng_key", (ctypes.c_uint32 * 8)(*RNG_KEY))
    monkeypatch.setattr(pk._key, "next_nonce", lambda: NONCE)
    ms, _ = _ms_rs(k, bits + 2)
    got, _ = pk.encrypt_encoded(_plain(ms, lp=pk._key.L1), True).to_signed_ints(pk.ns)
    rs = draw_below_host(RNG_KEY, NONCE, COUNT, k.n, pk._key.L2)
    assert all(1 <= r < k.n for r in rs)
    assert got == [ou_ref.encrypt(k, m, r) for m, r in zip(ms, rs)]


def test_two_encryptions_differ(objs):
    sk, pk, coder = objs[2048]
    pv = coder.encode_u64_vec([7] * COUNT, device="cuda")
    a, _ = pk.encrypt_encoded(pv, True).to_signed_ints(pk.ns)
    b, _ = pk.encrypt_encoded(pv, False).to_signed_ints(pk.ns)  # `obfuscate` is ignored: h^r always
    assert all(x != y for x, y in zip(a, b)) and len(set(a)) == COUNT
    assert coder.decode_u64_vec(sk.decrypt_to_encoded(pk.encrypt_encoded(pv, True))) == [7] * COUNT


@pytest.mark.parametrize("bits", [1540, 2048, 3072])
def test_modulus_only_ops(objs, bits):
    k = KEYS[bits]
    sk, pk, coder = objs[bits]
    rng = random.Random(bits + 3)
    ms, rs = _ms_rs(k, bits + 3)
    ms = [m % (1 << 60) for m in ms]
    ea = [rng.choice([0, 0, 1, 2]) for _ in range(COUNT)]
    eb = [rng.choice([0, 1, 3]) for _ in range(COUNT)]
    a = _encrypt(objs, bits, ms, rs, ea)
    b = _encrypt(objs, bits, ms[::-1], rs[::-1], eb)
    ca = [ou_ref.encrypt(k, m, r) for m, r in zip(ms, rs)]
    cb = ca[::-1]
    # add with equal and unequal exponents
    got = a.add(pk, b).to_signed_ints(pk.ns)
    want = [ou_ref.add(k, (x, e), (y, f)) for x, e, y, f in zip(ca, ea, cb, eb)]
    assert got == ([w[0] for w in want], [w[1] for w in want])
    # the literal 1 on either side
    ones = ou.CiphertextVector.zeros(COUNT, device="cuda")
    assert ones.add(pk, a).to_signed_ints(pk.ns) == (ca, ea)
    assert a.add(pk, ou.CiphertextVector.zeros(COUNT, device="cuda")).to_signed_ints(pk.ns) == (ca, ea)
    # neg, sub
    assert a.neg(pk).to_signed_ints(pk.ns) == ([ou_ref.neg(k, c) for c in ca], ea)
    a0 = _encrypt(objs, bits, ms, rs)
    b0 = _encrypt(objs, bits, ms[::-1], rs[::-1])
    assert a0.sub(pk, b0).to_signed_ints(pk.ns)[0] == [x * ou_ref.neg(k, y) % k.n for x, y in zip(ca, cb)]
    # mul by plaintexts up to 64 bits, 0 and 1 included: plain c^pt mod n
    pts = [0, 1, 2 ** 64 - 1, 2, 3] + [rng.randrange(2 ** 64) for _ in range(COUNT - 5)]
    got = a0.mul(pk, _plain(pts)).to_signed_ints(pk.ns)[0]
    assert got == [ou_ref.mul(k, c, t) for c, t in zip(ca, pts)]
    # idouble
    d = _encrypt(objs, bits, ms, rs)
    d.idouble(pk)
    assert d.to_signed_ints(pk.ns)[0] == [c * c % k.n for c in ca]
    # one iupdate: 67 samples x 3 positions into 8 slots
    pos = [[rng.randrange(8) for _ in range(3)] for _ in range(COUNT)]
    hist = ou.CiphertextVector.zeros(8, device="cuda")
    hist.iupdate(a0, pos, 1, pk)
    want = [1] * 8
    for c, row in zip(ca, pos):
        for s in row:
            want[s] = want[s] * c % k.n
    assert hist.to_signed_ints(pk.ns)[0] == want


@pytest.mark.parametrize("bits", [1542, 3072])
def test_neg_sub_batch_inversion(objs, bits):
    """fphe_neg from 4096 elements: k_binv_pre27, k_ou_inv27 over the group totals, k_binv_post27."""
    k = KEYS[bits]
    sk, pk, coder = objs[bits]
    rng = random.Random(bits + 4)
    count = 4096 + COUNT
    cs = [1, k.n - 1, k.g] + [1 + rng.randrange(k.n - 1) for _ in range(count - 3)]
    a = ou.CiphertextVector.from_signed_ints(cs, [0] * count, k.n, device="cuda")
    inv = [ou_ref.neg(k, c) for c in cs]
    assert a.neg(pk).to_signed_ints(pk.ns)[0] == inv
    b = ou.CiphertextVector.from_signed_ints(cs[::-1], [0] * count, k.n, device="cuda")
    assert b.sub(pk, a).to_signed_ints(pk.ns)[0] == [x * y % k.n for x, y in zip(cs[::-1], inv)]


def test_secureboost_flow_through_protocol_ou(objs):
    bits = 2048
    k = KEYS[bits]
    sk, pk, coder = protocol_ou.from_keys(*objs[bits])
    ev = protocol_ou.evaluator
    rng = random.Random(99)
    OFF, PREC = 64, 30
    gh = [rng.uniform(0, 1000) for _ in range(2 * COUNT)]  # (g, h) per sample, packed in one plaintext
    packed = coder.pack_floats(torch.tensor(gh, dtype=torch.float64, device="cuda"), OFF, 2, PREC)
    ints = ou_ref.pack_floats(gh, OFF, 2, PREC)
    assert packed.to_ints()[0] == ints
    ct = pk.encrypt_encoded(packed, True)
    pos = [[rng.randrange(4), 4 + rng.randrange(4)] for _ in range(COUNT)]  # 2 features x 4 bins
    hist = ev.zeros(8, None)
    ev.i_update(pk, hist, ct, pos, 1)
    ev.chunking_cumsum_with_step(pk, hist, [4, 4], 1)
    sq = ev.pack_squeeze(hist, 2, 2 * OFF, pk)
    dec = sk.decrypt_to_encoded(sq)
    # the same arithmetic on the packed integers
    h = [0] * 8
    for v, row in zip(ints, pos):
        for s in row:
            h[s] += v
    for c0 in (0, 4):
        for j in range(1, 4):
            h[c0 + j] += h[c0 + j - 1]
    want = [(h[2 * i] << (2 * OFF)) + h[2 * i + 1] for i in range(4)]
    assert dec.to_ints()[0] == want
    floats = ou_ref.unpack_floats(want, OFF, 4, PREC, 16)
    assert coder.coder.unpack_floats(dec, OFF, 4, PREC, 16) == floats  # float64, ==
    # the adapter returns torch.tensor(list), a float32 tensor, as the reference's ou.py:59-60
    assert torch.equal(coder.unpack_floats(dec, OFF, 4, PREC, 16), torch.tensor(floats))


def test_guards(objs):
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    k = KEYS[1024]
    sk, pk, coder = objs[1024]
    octx, osk = pk._key.ctx(dev), sk._key.ctx(dev)
    L2, L1 = pk._key.L2, pk._key.L1
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    b8 = torch.zeros(64, dtype=torch.uint8, device=dev)
    Pm, C, R = z(1, L1, 64), z(1, L2, 64), z(1, L2, 64)
    R[:, 0, :] = 1
    key = (ctypes.c_uint32 * 8)(*RNG_KEY)
    ptr = P._ptr
    assert lib.fphe_encrypt(octx, ptr(Pm), L1, ptr(b8), 1, 1, None, key, 1, ptr(C), ptr(b8), None) == _lib.FPHE_ERR_ARG
    assert lib.fphe_decrypt(osk, ptr(C), 1, ptr(Pm), None) == _lib.FPHE_ERR_ARG
    assert lib.fphe_ou_decrypt(octx, ptr(C), 1, ptr(Pm), None) == _lib.FPHE_ERR_NO_SK
    assert lib.fphe_ou_encrypt(octx, ptr(Pm), L1, 1, ptr(R), key, 1, ptr(C), None) == _lib.FPHE_OK
    with open(os.path.join(ou_ref.HERE, "golden", "paillier_1024.json")) as f:
        fx = json.load(f)
    psk, ppk, pcoder = P.keypair_from_primes(int(fx["p"], 16), int(fx["q"], 16))
    pctx = ppk._key.ctx(dev)
    Cp = z(1, ppk._key.L2, 64)
    assert lib.fphe_ou_encrypt(pctx, ptr(Pm), 1, 1, None, key, 1, ptr(Cp), None) == _lib.FPHE_ERR_ARG
    assert lib.fphe_ou_decrypt(pctx, ptr(Cp), 1, ptr(Pm), None) == _lib.FPHE_ERR_ARG
    torch.cuda.synchronize()

    def create(n, g, h, p=None, q=None, bits=1024):
        w = lambda v, L: (ctypes.c_uint32 * L)(*P.ints_to_limbs([v], L)[0].tolist())
        out = ctypes.c_void_p()
        st = lib.fphe_ou_ctx_create(dev.index, bits, w(n, L2), w(g, L2), w(h, L2),
                                    None if p is None else w(p, L1), None if q is None else w(q, L1), ctypes.byref(out))
        if st == _lib.FPHE_OK:
            lib.fphe_ctx_destroy(out)
        return st
    assert create(k.n, k.g, k.h, k.p, k.q) == _lib.FPHE_OK
    assert create(k.n + 1, k.g, k.h) == _lib.FPHE_ERR_KEY                      # even n
    assert create(k.n, k.g, k.h, k.p, k.p) == _lib.FPHE_ERR_KEY                # p == q
    assert create(k.n + 2, k.g, k.h, k.p, k.q) == _lib.FPHE_ERR_KEY            # n != p^2 q
    assert create(k.n, 0, k.h) == _lib.FPHE_ERR_KEY and create(k.n, k.g, k.n) == _lib.FPHE_ERR_KEY
    assert create(k.n, k.g, k.h, bits=1026) == _lib.FPHE_ERR_KEY               # bits(n) != key_bits
    assert create(k.n, k.g, k.h, bits=512) == _lib.FPHE_ERR_ARG
