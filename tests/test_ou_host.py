"""CPU checks of the Okamoto-Uchiyama surface (fate_amd.ou): key generation by the reference's
loops (ou/src/lib.rs:69-91), the oracle of the GPU tests on the committed keys, the pyo3 method
names of fate_utils/src/ou/ou.rs, and the packed-float codec's host restatement."""
import random

import pytest

from fate_amd import _lib, ou
from tests import ou_ref

KEYS = ou_ref.load_keys()


def test_keygen_params_follow_the_reference():
    bits = 1024
    p, q, g = ou.keygen_params(bits)
    n = p * p * q
    assert n.bit_length() == bits and p != q
    assert p.bit_length() >= bits // 3 and q.bit_length() >= bits - 2 * (bits // 3)
    assert 1 <= g < n and pow(g, p - 1, p * p) != 1
    # the key objects the product builds from them (no device needed to construct them)
    sk, pk, coder = ou.keypair_from_primes(p, q, g)
    assert (pk.n, pk.g) == (n, g) and pk.h == pow(g, n, n) and sk.h == pk.h
    assert (sk.p, sk.q, sk.g) == (p, q, g) and coder.n == n
    assert pk._key.L2 == 64 and pk._key.L1 == 32 and pk._key.modulus == n and sk._key.p == p
    k = ou_ref.Key(p, q, g)
    assert ou_ref.decrypt(k, ou_ref.encrypt(k, 12345, 67890)) == 12345
    with pytest.raises(ValueError):  # g of order dividing p - 1 mod p^2
        ou.keypair_from_primes(p, q, 1)


def test_coder_without_its_key_says_so():
    c = ou.Coder(12345)
    for call in (lambda: c.pack_floats([1.0], 64, 1, 30, device="cpu"), lambda: c._key):
        with pytest.raises(ValueError, match="no OU key"):
            call()


@pytest.mark.parametrize("bits", sorted(KEYS))
def test_fixture_keys_round_trip(bits):
    k = KEYS[bits]
    assert k.n.bit_length() == bits and k.p != k.q and pow(k.g, k.p - 1, k.p2) != 1
    rng = random.Random(bits)
    for m in (0, 1, 2 ** 64 - 1, k.p - 1, rng.randrange(k.p)):
        r = 1 + rng.randrange(k.n - 1)
        c = ou_ref.encrypt(k, m, r)
        assert ou_ref.decrypt(k, c) == m
        c2 = ou_ref.encrypt(k, 5, 1 + rng.randrange(k.n - 1))
        if m + 5 < k.p:
            assert ou_ref.decrypt(k, c * c2 % k.n) == m + 5
    assert ou_ref.decrypt(k, 1) == 0 and ou_ref.decrypt(k, k.g) == 1


def test_unsupported_sizes():
    assert ou.supports(1024) and ou.supports(1540) and ou.supports(4096)
    assert not ou.supports(512) and not ou.supports(1025) and not ou.supports(4098)
    with pytest.raises(ValueError):
        ou.keygen(512)
    assert ou.limbs_for(2048) == 64 and ou.limbs_for(2050) == 128


# the pyo3 methods of fate_utils.ou (fate_utils/src/ou/ou.rs:212-386, 100-204)
CIPHERTEXT_VECTOR_METHODS = [
    "zeros", "pack_squeeze", "slice", "slice_indexes", "cat", "i_shuffle", "shuffle", "intervals_slice",
    "iadd_slice", "iadd_vec_self", "isub_vec_self", "iadd_vec", "isub_vec", "iupdate", "iupdate_with_masks",
    "iadd", "idouble", "chunking_cumsum_with_step", "intervals_sum_with_step", "tolist", "add", "add_scalar",
    "sub", "sub_scalar", "rsub", "rsub_scalar", "mul", "mul_scalar", "matmul", "rmatmul", "__len__", "__str__",
]
CODER_METHODS = ["encode_u64", "decode_u64", "encode_u32", "decode_u32", "pack_floats", "unpack_floats",
                 "encode_u64_vec", "decode_u64_vec", "encode_u32_vec", "decode_u32_vec"]


def test_pyo3_method_names():
    for name in CIPHERTEXT_VECTOR_METHODS:
        assert callable(getattr(ou.CiphertextVector, name)), name
    for name in CODER_METHODS:
        assert callable(getattr(ou.Coder, name)), name
    for name in ("encrypt_encoded", "encrypt_encoded_scalar"):
        assert callable(getattr(ou.PK, name))
    for name in ("decrypt_to_encoded", "decrypt_to_encoded_scalar"):
        assert callable(getattr(ou.SK, name))
    assert callable(ou.Evaluator.cat) and callable(ou.Evaluator.slice_indexes) and callable(ou.keygen)
    from fate_amd import protocol_ou
    assert callable(protocol_ou.keygen) and callable(protocol_ou.evaluator.i_update)
    assert callable(protocol_ou.evaluator.pack_squeeze) and callable(protocol_ou.evaluator.zeros)


def test_header_and_bindings_name_the_ou_entry_points():
    for name in ("fphe_ou_ctx_create", "fphe_ou_encrypt", "fphe_ou_decrypt"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_pack_unpack_oracle_on_exact_vectors():
    """The packed-float oracle (tests/ou_ref.py) against a restatement of fixedpoint_ou/src/lib.rs:
    69-108 on dyadic inputs, where v 2^precision is an integer and nothing rounds: exact.  This
    pins the oracle only; ou.Coder.pack_floats / unpack_floats run on the device and are checked
    against this oracle in tests/test_gpu_ou.py (the SecureBoost-shaped flow)."""
    rng = random.Random(5)
    for offset_bit, pack_num, precision in ((64, 2, 30), (40, 5, 20), (100, 3, 52)):
        ints = [rng.randrange(1 << min(offset_bit - 4, 60)) for _ in range(2 * pack_num + 1)] + [0, 1]
        xs = [i / 2 ** precision for i in ints]  # exact in float64 (< 2^53 significant bits or dyadic)
        ints = [int(x * 2 ** precision) for x in xs]
        packed = ou_ref.pack_floats(xs, offset_bit, pack_num, precision)
        want = []
        for c0 in range(0, len(ints), pack_num):
            w = 0
            for i in ints[c0:c0 + pack_num]:
                w = (w << offset_bit) + i
            want.append(w)
        assert packed == want
        assert ou_ref.unpack_floats(packed, offset_bit, pack_num, precision, len(xs)) == xs
    # round half away from zero (MPFR round), and field sums unpack to the sums of the fields
    assert ou_ref.pack_floats([0.5, 1.5, 2.5], 8, 3, 0) == [(1 << 16) + (2 << 8) + 3]
    a = ou_ref.pack_floats([1.5, 2.25], 64, 2, 30)[0]
    b = ou_ref.pack_floats([0.5, 0.75], 64, 2, 30)[0]
    assert ou_ref.unpack_floats([a + b], 64, 2, 30, 2) == [2.0, 3.0]
