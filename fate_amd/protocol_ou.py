"""Drop-in replacement for ``fate.arch.protocol.phe.ou`` on MI355X.

Mirrors python/fate/arch/protocol/phe/ou.py (SK / PK / Coder wrappers, ``keygen(key_size)`` and
the ``evaluator`` plugin) over :mod:`fate_amd.ou`, in the pass-through style of
:mod:`fate_amd.protocol`.  FATE's ``CipherKit.phe`` reaches it for ``kind: ou``
(python/fate/arch/context/_cipher.py:103-149); see INTEGRATION.md.  The evaluator is
:class:`fate_amd.protocol.evaluator` itself -- every method takes the key and runs mod n on an
OU key -- with ``zeros`` at OU's ciphertext width.
"""
from __future__ import annotations

import torch

from . import ou as _ou
from . import protocol as _proto
from .paillier import CiphertextVector, PlaintextVector

V = torch.Tensor
EV = CiphertextVector
FV = PlaintextVector

SK = _proto.SK
PK = _proto.PK

# dtype -> the fate_utils.ou Coder method suffix (ou.py:127-171: the i64 / i32 names map to the
# unsigned encoders; the float encoders are commented out in the reference)
_SUFFIX = {torch.int64: "u64", torch.int32: "u32"}


def _suffix(dtype) -> str:
    if dtype not in _SUFFIX:
        raise NotImplementedError(f"{dtype} not supported")
    return _SUFFIX[dtype]


class Coder:
    def __init__(self, coder: _ou.Coder):
        self.coder = coder

    def pack_floats(self, float_tensor: V, offset_bit: int, pack_num: int, precision: int) -> FV:
        return self.coder.pack_floats(float_tensor.detach(), offset_bit, pack_num, precision)

    def unpack_floats(self, packed: FV, offset_bit: int, pack_num: int, precision: int, total_num: int) -> V:
        return torch.tensor(self.coder.unpack_floats(packed, offset_bit, pack_num, precision, total_num))

    def encode_tensor(self, tensor: V, dtype: torch.dtype = None) -> FV:
        return self.encode_vec(tensor.flatten(), dtype=tensor.dtype)

    def decode_tensor(self, tensor: FV, dtype: torch.dtype, shape: torch.Size = None, device=None) -> V:
        data = self.decode_vec(tensor, dtype)
        if shape is not None:
            data = data.reshape(shape)
        if device is not None:
            data = data.to(device.to_torch_device() if hasattr(device, "to_torch_device") else device)
        return data

    def encode_vec(self, vec: V, dtype: torch.dtype = None) -> FV:
        dtype = vec.dtype if dtype is None else dtype
        return getattr(self.coder, f"encode_{_suffix(dtype)}_vec")(vec.detach().flatten().cpu())

    def decode_vec(self, vec: FV, dtype: torch.dtype) -> V:
        return torch.tensor(getattr(self.coder, f"decode_{_suffix(dtype)}_vec")(vec))

    def encode(self, val, dtype=None):
        if isinstance(val, torch.Tensor):
            assert val.ndim == 0, "only scalar supported"
            dtype = val.dtype
            val = val.item()
        return getattr(self.coder, f"encode_{_suffix(dtype)}")(val)

    def encode_i64(self, val: int):
        return self.coder.encode_u64(val)

    def decode_i64(self, val):
        return self.coder.decode_u64(val)

    def encode_i32(self, val: int):
        return self.coder.encode_u32(val)

    def decode_i32(self, val):
        return self.coder.decode_u32(val)

    def encode_i64_vec(self, vec: V):
        return self.encode_vec(vec, torch.int64)

    def decode_i64_vec(self, vec):
        return self.decode_vec(vec, torch.int64)

    def encode_i32_vec(self, vec: V):
        return self.encode_vec(vec, torch.int32)

    def decode_i32_vec(self, vec):
        return self.decode_vec(vec, torch.int32)


def supports(key_size: int) -> bool:
    """Whether this backend runs OU keys of ``key_size`` bits (even, 1024..4096)."""
    return _ou.supports(key_size)


def keygen(key_size):
    """ou.py:174-176.  ValueError for sizes :func:`supports` rejects."""
    sk, pk, coder = _ou.keygen(key_size)
    return SK(sk), PK(pk), Coder(coder)


def from_keys(sk: _ou.SK, pk: _ou.PK, coder: _ou.Coder):
    """The wrappers of existing :mod:`fate_amd.ou` key objects."""
    return SK(sk), PK(pk), Coder(coder)


class evaluator(_proto.evaluator):
    """ou.py:179-400: the methods of :class:`fate_amd.protocol.evaluator`."""

    @staticmethod
    def zeros(size, dtype) -> EV:
        return _ou.CiphertextVector.zeros(size)
