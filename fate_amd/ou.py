"""Okamoto-Uchiyama on the device: the surface of ``fate_utils.ou``
(rust/fate_utils/crates/fate_utils/src/ou/ou.rs; scheme crates/ou/src/lib.rs:69-138,
fixed-point layer crates/fixedpoint_ou/src/lib.rs).

n = p^2 q, h = g^n mod n, encrypt(m) = g^m h^r mod n, decrypt(c) = L(c^(p-1) mod p^2)
L(g^(p-1) mod p^2)^-1 mod p.  Plaintexts are unsigned; ciphertexts live mod n, so a 2048-bit
OU key runs the kernels a 1024-bit Paillier key runs (64-word ciphertexts).

The vector classes are :mod:`fate_amd.paillier`'s: every vector method takes the ``PK`` and
reaches the device through ``pk._key``, and an OU ``PK`` carries an OU device context
(``fphe_ou_ctx_create``) on which the modulus-only entry points compute mod n.  Only key
objects, the coder and the two constructors that know no key (``zeros``,
``from_signed_ints``) are restated here.
"""
from __future__ import annotations

import ctypes
import secrets
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _keygen, _lib
from . import paillier as _P
from .paillier import (Ciphertext, Evaluator, PanicException, Plaintext, PlaintextVector,  # noqa: F401
                       WAVE, _ntiles, _ptr, _stream, ints_to_limbs, rows_to_tiles)

MIN_KEY_BITS, MAX_KEY_BITS = 1024, 4096  # 1024: FATE's minimum_key_size for `ou`


def supports(key_bits: int) -> bool:
    return MIN_KEY_BITS <= key_bits <= MAX_KEY_BITS and key_bits % 2 == 0


def limbs_for(key_bits: int) -> int:
    """Ciphertext words (L2) of an OU key: n zero-padded to 64 words up to 2048 bits, else 128."""
    return 64 if key_bits <= 2048 else 128


class _OuKeyCtx(_P._KeyCtx):
    """One fphe_ctx per HIP device for an OU key (fphe_ou_ctx_create)."""

    def __init__(self, n: int, g: int, h: int, p: Optional[int] = None, q: Optional[int] = None):
        self.n, self.g, self.h, self.p, self.q = n, g, h, p, q
        self.key_bits = n.bit_length()
        if not supports(self.key_bits):
            raise ValueError(f"unsupported OU key size {self.key_bits}: this backend runs even sizes "
                             f"{MIN_KEY_BITS}..{MAX_KEY_BITS}")
        self.L2 = limbs_for(self.key_bits)
        self.L1 = self.L2 // 2  # plaintext words (m < p, a third of n's bits)
        self.modulus = n
        self._setup()

    def _create(self, lib, idx: int) -> ctypes.c_void_p:
        def words(v, L):
            return (ctypes.c_uint32 * L)(*ints_to_limbs([v], L)[0].tolist())
        pw = qw = None
        if self.p is not None:
            pw, qw = words(self.p, self.L1), words(self.q, self.L1)
        out = ctypes.c_void_p()
        _lib.check(lib.fphe_ou_ctx_create(idx, self.key_bits, words(self.n, self.L2), words(self.g, self.L2),
                                          words(self.h, self.L2), pw, qw, ctypes.byref(out)), "fphe_ou_ctx_create")
        return out


def _key_for(n: int, g: int, h: int, p: Optional[int] = None, q: Optional[int] = None) -> _OuKeyCtx:
    """The public context of a key is registered under its modulus, so that the vectors of
    :mod:`fate_amd.paillier` (which carry only the modulus) find it; a private one is kept
    beside the Paillier keys."""
    with _P._KEYS_LOCK:
        if p is None:
            k = _P._SCHEME_KEYS.get(n)
            if k is None:
                k = _P._SCHEME_KEYS[n] = _OuKeyCtx(n, g, h)
                _P._KEYS[(n, None)] = k  # torn down with the others at exit
            elif (k.g, k.h) != (g, h):
                raise ValueError("another OU key with this modulus is already in use")
            return k
        k = _P._KEYS.get((n, p))
        if k is None:
            k = _P._KEYS[(n, p)] = _OuKeyCtx(n, g, h, p, q)
        return k


class CiphertextVector(_P.CiphertextVector):
    """``fate_utils.ou.CiphertextVector``: :class:`fate_amd.paillier.CiphertextVector` with the
    two key-less constructors at OU's widths.  Operations return the base class, which is the
    same object layout."""

    __slots__ = ()

    @staticmethod
    def zeros(size: int, L2: int = 64, device=None) -> _P.CiphertextVector:
        return _P.CiphertextVector.zeros(size, L2, device)

    @staticmethod
    def from_signed_ints(cs: Sequence[int], exps: Sequence[int], n: int, L2: Optional[int] = None,
                         device=None) -> _P.CiphertextVector:
        """Ciphertext integers (|c| < n) under the registered OU key of modulus n."""
        if n not in _P._SCHEME_KEYS:
            raise ValueError("from_signed_ints: no OU key with this modulus (make its PK first)")
        L2 = _P._SCHEME_KEYS[n].L2 if L2 is None else L2
        dev = _P._device(device)
        count = len(cs)
        C = torch.from_numpy(rows_to_tiles(ints_to_limbs([abs(c) for c in cs], L2)).view(np.int32)).to(dev)
        sign = _P._pad_flat(torch.tensor([1 if c < 0 else 0 for c in cs], dtype=torch.uint8), count).to(dev)
        ex = _P._pad_flat(torch.tensor(list(exps), dtype=torch.int32), count).to(dev)
        v = _P.CiphertextVector(C, sign, ex, count, None, raw=True)
        _P._resolve(v, n)
        return v


class PK(_P.PK):
    """``fate_utils.ou.PK`` (ou.rs:48-74; ou::PK {n, g, h})."""

    def __init__(self, n: Optional[int] = None, g: Optional[int] = None, h: Optional[int] = None):
        self.n = n
        self._priv = None
        if n is not None:
            if g is None or h is None:  # paillier's internals rebuild a PK from a vector's modulus
                k = _P._SCHEME_KEYS.get(n)
                if k is None:
                    raise ValueError("ou.PK(n): no OU key with this modulus")
                g, h = k.g, k.h
            self._init_ou(n, g, h)

    def _init_ou(self, n: int, g: int, h: int):
        self.n, self.g, self.h = n, g, h
        self.ns = n  # the ciphertext modulus, where paillier.PK has n^2
        self._key = _key_for(n, g, h)

    @property
    def keyholder(self) -> bool:
        return False  # no key-holder (CRT) encrypt for OU

    def encrypt_encoded(self, plaintext_vector: PlaintextVector, obfuscate: bool,
                        *, r: Optional[Sequence[int]] = None) -> _P.CiphertextVector:
        """``PK.encrypt_encoded`` (ou.rs:50-56 -> ou/src/lib.rs:100-108).  `obfuscate` is ignored
        as in the reference (h^r is always applied, lib.rs:103).  ``r`` (our extension) injects
        the nonces (parity mode); default draws them on the device."""
        pv = plaintext_vector
        dev = pv.device
        k = self._key
        n = pv.count
        out = _P.CiphertextVector.empty(n, k.L2, dev)
        out.n = self.n
        if n == 0:
            return out
        if pv.lp > k.L1:
            raise PanicException("plaintext does not fit the key")
        rt = None
        if r is not None:
            if len(r) != n:
                raise ValueError("need one r per element")
            rt = torch.from_numpy(rows_to_tiles(ints_to_limbs(list(r), k.L2)).view(np.int32)).to(dev)
        _lib.check(_lib.load().fphe_ou_encrypt(k.ctx(dev), _ptr(pv.P), pv.lp, n, _ptr(rt), k.rng_key, k.next_nonce(),
                                               _ptr(out.C), ctypes.c_void_p(_stream(dev))), "fphe_ou_encrypt")
        out.exp[:n] = pv.exp[:n]
        out.ebound = pv.ebound
        return out

    def encrypt_encoded_scalar(self, plaintext: Plaintext, obfuscate: bool) -> Ciphertext:
        return Ciphertext(self.encrypt_encoded(plaintext.vec, obfuscate))

    # the bincode pickles of OU keys are deferred: a plain tuple state
    def __getstate__(self):
        return (self.n, self.g, self.h)

    def __setstate__(self, state):
        self._priv = None
        self._init_ou(*state)


class SK:
    """``fate_utils.ou.SK`` (ou.rs:76-98; ou::SK {p, p_minus_one, q, g})."""

    def __init__(self, p: Optional[int] = None, q: Optional[int] = None, g: Optional[int] = None):
        if p is not None:
            self._init(p, q, g)

    def _init(self, p: int, q: int, g: int):
        if p == q:
            raise PanicException("p == q")
        self.p, self.q, self.g = p, q, g
        self.n = p * p * q
        self.h = pow(g, self.n, self.n)
        _key_for(self.n, g, self.h)  # the public context the vectors resolve against
        self._key = _key_for(self.n, g, self.h, p, q)

    def decrypt_to_encoded(self, data: _P.CiphertextVector) -> PlaintextVector:
        """``SK.decrypt_to_encoded`` (ou.rs:78-80 -> ou/src/lib.rs:120-131): m in [0, p)."""
        dev = data.device
        k = self._key
        _P._resolve(data, self.n)
        data = _P._fit_limbs(data, k.L2)
        n = data.count
        nt = _ntiles(n)
        P = torch.empty((nt, k.L1, WAVE), dtype=torch.int32, device=dev)
        out = PlaintextVector(P, torch.zeros(nt * WAVE, dtype=torch.uint8, device=dev), data.exp.clone(), n)
        if n == 0:
            return out
        _lib.check(_lib.load().fphe_ou_decrypt(k.ctx(dev), _ptr(data.C), n, _ptr(P), ctypes.c_void_p(_stream(dev))),
                   "fphe_ou_decrypt")
        return out

    def decrypt_to_encoded_scalar(self, data: Ciphertext) -> Plaintext:
        return Plaintext(self.decrypt_to_encoded(data.vec))

    def __getstate__(self):
        return (self.p, self.q, self.g)

    def __setstate__(self, state):
        self._init(*state)


class Coder:
    """``fate_utils.ou.Coder`` (ou.rs:100-204; fixedpoint_ou::Coder lib.rs:55-126): unsigned
    integers and packed floats only (the reference has float and signed encode commented out)."""

    def __init__(self, n: Optional[int] = None):
        self.n = n

    @property
    def _key(self) -> _OuKeyCtx:
        """The key's public context, looked up when first needed: a coder may be made (or
        unpickled) before its key's PK."""
        k = _P._SCHEME_KEYS.get(self.n) if self.n is not None else None
        if k is None:
            raise ValueError("ou.Coder: no OU key with this coder's modulus yet (make or unpickle its PK first, "
                             "or use the coder keygen returns)")
        return k

    def __getstate__(self):
        return (self.n,)

    def __setstate__(self, state):
        self.__init__(*state)

    def _encode(self, data, bits: int, device=None) -> PlaintextVector:
        vals = [int(v) for v in (data.tolist() if hasattr(data, "tolist") else data)]
        for v in vals:
            if not 0 <= v < (1 << bits):
                raise OverflowError(f"encode_u{bits}: {v} out of range")
        out = PlaintextVector.from_ints(vals, [0] * len(vals), device=device, lp=2)
        out.ebound = (0, 0)
        return out

    def encode_u64_vec(self, data, device=None) -> PlaintextVector:
        return self._encode(data, 64, device)

    def encode_u32_vec(self, data, device=None) -> PlaintextVector:
        return self._encode(data, 32, device)

    def _decode(self, data: PlaintextVector, bits: int) -> List[int]:
        # decode_u64 (lib.rs:115-119): (mantissa << 4 exp).to_i128() as u64 (rug's floor shift for
        # exp < 0); decode_u32 is that value `as u32`
        sig, exp = data.to_ints()
        out = []
        for s, e in zip(sig, exp):
            v = s << (4 * e) if e >= 0 else s >> (-4 * e)
            if v >= 1 << 127:
                raise PanicException("cant't convert to i128")
            out.append(v & ((1 << bits) - 1))
        return out

    def decode_u64_vec(self, data: PlaintextVector) -> List[int]:
        return self._decode(data, 64)

    def decode_u32_vec(self, data: PlaintextVector) -> List[int]:
        return self._decode(data, 32)

    def encode_u64(self, data: int) -> Plaintext:
        return Plaintext(self.encode_u64_vec([data]))

    def encode_u32(self, data: int) -> Plaintext:
        return Plaintext(self.encode_u32_vec([data]))

    def decode_u64(self, data: Plaintext) -> int:
        return self.decode_u64_vec(data.vec)[0]

    def decode_u32(self, data: Plaintext) -> int:
        return self.decode_u32_vec(data.vec)[0]

    def pack_floats(self, float_tensor, offset_bit: int, pack_num: int, precision: int,
                    device=None) -> PlaintextVector:
        """``Coder.pack_floats`` (ou.rs:136-139; fixedpoint_ou lib.rs:69-84), on the device
        (fphe_pack_f64 reads no key).  Packed values are unsigned: a negative sum panics."""
        L1 = self._key.L1
        dev = _P._device(device if device is not None else (float_tensor.device if torch.is_tensor(float_tensor)
                                                            and float_tensor.is_cuda else None))
        x = torch.as_tensor(float_tensor).detach().flatten().to(dtype=torch.float64, device=dev).contiguous()
        n = (x.numel() + pack_num - 1) // pack_num
        nt = _ntiles(n)
        out = PlaintextVector(torch.zeros((nt, L1, WAVE), dtype=torch.int32, device=dev),
                              torch.zeros(nt * WAVE, dtype=torch.uint8, device=dev),
                              torch.zeros(nt * WAVE, dtype=torch.int32, device=dev), n)
        if n == 0:
            return out
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().fphe_pack_f64(self._key.ctx(dev), _ptr(x), x.numel(), offset_bit, pack_num, precision,
                                             _ptr(out.P), _ptr(out.neg), _ptr(out.exp), _ptr(err),
                                             ctypes.c_void_p(_stream(dev))), "fphe_pack_f64")
        _P._raise_err(err)
        if bool(out.neg.any()):
            raise PanicException("pack_floats: negative packed value (OU plaintexts are unsigned)")
        out.ebound = (0, 0)
        return out

    def unpack_floats(self, packed: PlaintextVector, offset_bit: int, pack_num: int, precision: int,
                      total_num: int) -> List[float]:
        """``Coder.unpack_floats`` (ou.rs:141-143; lib.rs:85-108), on the device."""
        key, dev = self._key, packed.device
        out = torch.zeros(total_num, dtype=torch.float64, device=dev)
        if total_num and packed.count:
            _lib.check(_lib.load().fphe_unpack_f64(key.ctx(dev), _ptr(packed.P), packed.P.shape[1],
                                                   packed.count, offset_bit, pack_num, precision, total_num, _ptr(out),
                                                   ctypes.c_void_p(_stream(dev))), "fphe_unpack_f64")
        return out.cpu().tolist()


def keypair_from_primes(p: int, q: int, g: int) -> Tuple[SK, PK, Coder]:
    """The key objects of given (p, q, g): n = p^2 q, h = g^n mod n (ou/src/lib.rs:89-90)."""
    n = p * p * q
    if not 1 <= g < n or pow(g, p - 1, p * p) == 1:
        raise ValueError("g must be in [1, n-1] with g^(p-1) mod p^2 != 1")
    sk = SK(p, q, g)
    pk = PK(n, g, sk.h)
    return sk, pk, Coder(n)


def keygen_params(bit_length: int) -> Tuple[int, int, int]:
    """(p, q, g) by the reference's loops (ou/src/lib.rs:70-88): p of bit_length / 3 bits, q of
    the rest, until p != q and bits(p^2 q) == bit_length; g = gen_positive_integer(n - 1) + 1
    until g^(p-1) mod p^2 != 1."""
    pb = bit_length // 3
    while True:
        p = _keygen.gen_prime(pb)
        q = _keygen.gen_prime(bit_length - 2 * pb)
        n = p * p * q
        if p != q and n.bit_length() == bit_length:
            break
    while True:
        g = secrets.randbelow(n - 1) + 1
        if pow(g, p - 1, p * p) != 1:
            return p, q, g


def keygen(bit_length: int) -> Tuple[SK, PK, Coder]:
    """``fate_utils.ou.keygen`` (ou.rs:206-209)."""
    if not supports(bit_length):
        raise ValueError(f"unsupported OU key size {bit_length}")
    return keypair_from_primes(*keygen_params(bit_length))
