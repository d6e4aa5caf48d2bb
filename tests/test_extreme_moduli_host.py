"""The key blob of every extreme key (tests/golden/extreme_keys.json; DESIGN.md "Extreme moduli")
against plain Python integers: each modulus in its engine radix with R^k mod N and -N^-1 mod 2^LB,
the 32-bit CRT constants, the exponents, the scalars and OU's fixed-base tables.  The blob comes
from the stand-alone tests/key_blob_dump.cpp (fate_amd/csrc/key_blob.h and host_bn.h, no GPU).
tests/test_key_blob.py pins hashes of the random keys' blobs; this checks that the constants are
right where host_bn.h meets all-ones divisors, moduli that are 1 mod 2^32 and two-limb moduli."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OU_WIN = 4  # kOuWin (fate_amd/csrc/key_blob.h)

with open(os.path.join(GOLDEN, "extreme_keys.json")) as _f:
    FX = json.load(_f)


# fate_amd/csrc/radix.h, restated: a TPI's engine holds 37 tpi limbs of 28 bits (27 x 38 only at
# TPI 4 of a build with FPHE_RADIX4=27, which is not the default and not what this test compiles)
def rad_lb(tpi):
    return 28


def rad_ll(tpi):
    return 37


def _hx(v):
    return "-" if v is None else "%x" % v


def _cases():
    """{name: (line for the program, scheme, key dict of integers)}"""
    out = {}
    for name, k in sorted(FX["paillier"].items()):
        p, q = int(k["p"], 16), int(k["q"], 16)
        for sk in (False, True):
            nm = f"paillier_{name}_{'sk' if sk else 'pk'}"
            line = " ".join([nm, "paillier", str(k["bits"]), _hx(p * q), _hx(p if sk else None), _hx(q if sk else None)])
            out[nm] = (line, "paillier", dict(bits=k["bits"], p=p, q=q, sk=sk))
    for name, k in sorted(FX["ou_public"].items()):
        n, g, h = int(k["n"], 16), int(k["g"], 16), int(k["h"], 16)
        nm = f"ou_public_{name}"
        out[nm] = (" ".join([nm, "ou", str(k["bits"]), _hx(n), _hx(g), _hx(h), "-", "-"]), "ou",
                   dict(bits=k["bits"], n=n, g=g, h=h, p=None, q=None))
    for name, k in sorted(FX["ou_keys"].items()):
        p, q, g = int(k["p"], 16), int(k["q"], 16), int(k["g"], 16)
        n = p * p * q
        h = pow(g, n, n)
        for sk in (False, True):
            nm = f"ou_{name}_{'sk' if sk else 'pk'}"
            line = " ".join([nm, "ou", str(k["bits"]), _hx(n), _hx(g), _hx(h), _hx(p if sk else None), _hx(q if sk else None)])
            out[nm] = (line, "ou", dict(bits=k["bits"], n=n, g=g, h=h, p=p if sk else None, q=q if sk else None))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Build the program as tests/test_key_blob.py does and run it once over every case:
    {name: the parsed dump, with the blob as uint32 words under "blob"}."""
    tmp = tmp_path_factory.mktemp("extreme_blob")
    exe = tmp / "key_blob_dump"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "key_blob_dump.cpp")], check=True)
    lines = sorted((c[0] for c in CASES.values()), key=len, reverse=True)  # the widest keys first, spread out
    nproc = 8
    procs = []
    for i in range(nproc):
        (tmp / f"cases{i}.txt").write_text("\n".join(lines[i::nproc]) + "\n")
        procs.append(subprocess.Popen([str(exe), str(tmp / f"cases{i}.txt"), str(tmp)], stdout=subprocess.PIPE, text=True))
    stdout = ""
    for p in procs:
        stdout += p.communicate()[0]
        assert p.returncode == 0
    out, name, cur = {}, None, None
    for ln in stdout.splitlines():
        t = ln.split()
        if t[0] == "case":
            name, cur = t[1], {"status": int(t[3]), "ptr": {}, "val": {}, "ctx": {}}
            out[name] = cur
        elif t[0] in ("ptr", "val", "ctx"):
            cur[t[0]][t[1]] = int(t[2])
        elif t[0] == "end":
            cur["blob"] = np.fromfile(str(tmp / (name + ".blob")), dtype=np.uint32)
        else:
            cur[t[0]] = int(t[1])
    return out


def _words(v, n):
    """v as n little-endian 32-bit words"""
    return np.frombuffer(v.to_bytes(4 * n, "little"), dtype=np.uint32)


def _radix_rows(vals, nl, lb):
    """Each integer of vals as nl limbs of lb bits: [len(vals), nl] uint32."""
    nw = (nl * lb + 31) // 32 + 1
    w = np.stack([_words(v, nw) for v in vals]).astype(np.uint64)
    out = np.empty((len(vals), nl), dtype=np.uint32)
    for i in range(nl):
        k, off = (lb * i) >> 5, (lb * i) & 31
        x = w[:, k] | (w[:, k + 1] << np.uint64(32))
        out[:, i] = ((x >> np.uint64(off)) & np.uint64((1 << lb) - 1)).astype(np.uint32)
    return out


class Expect:
    """What a blob must hold: pointer fields as word arrays, scalar fields as integers.  check()
    also requires every KeyArgs field the program dumps to be either listed or null / zero, so a
    constant added to the blob later cannot go unchecked here."""

    def __init__(self):
        self.ptr, self.val, self.ctx = {}, {}, {}

    def words(self, field, v, n):
        assert 0 <= v < 1 << (32 * n), field
        self.ptr[field] = _words(v, n)

    def limbs(self, field, v, tpi):
        nl, lb = rad_ll(tpi) * tpi, rad_lb(tpi)
        assert 0 <= v < 1 << (lb * nl), field
        self.ptr[field] = _radix_rows([v], nl, lb)[0]

    def modulus(self, N, tpi, fN, r1, r2, r3, fnp):
        """put_modulus: N, R^k mod N for the fields given, -N^-1 mod 2^LB; R = 2^(LB NL)"""
        lb = rad_lb(tpi)
        R = 1 << (lb * rad_ll(tpi) * tpi)
        assert R >= 4 * N  # the lazy form's premise (mont_engine.inc)
        self.limbs(fN, N, tpi)
        for k, f in ((1, r1), (2, r2), (3, r3)):
            if f:
                self.limbs(f, pow(R, k, N), tpi)
        self.val[fnp] = (-pow(N, -1, 1 << lb)) % (1 << lb)
        assert (N * self.val[fnp] + 1) % (1 << lb) == 0

    def check(self, d, name):
        blob = d["blob"]
        assert d["status"] == 0 and d["blob_words"] == blob.size, name
        assert set(d["ptr"]) >= set(self.ptr) and set(d["val"]) >= set(self.val) and set(d["ctx"]) >= set(self.ctx), name
        for f, off in d["ptr"].items():
            if f not in self.ptr:
                assert off == -1, (name, f, "a section this test does not know")
                continue
            want = self.ptr[f]
            assert off >= 0 and off % 4 == 0 and off + want.size <= blob.size, (name, f)
            got = blob[off:off + want.size]
            assert np.array_equal(got, want), (name, f, [hex(int(x)) for x in got[:4]], [hex(int(x)) for x in want[:4]])
        for f, v in d["val"].items():
            assert v == self.val.get(f, 0), (name, f, hex(v))
        for f, v in self.ctx.items():
            assert d["ctx"][f] == v, (name, f)


def _inv32(N):
    return (-pow(N, -1, 1 << 32)) % (1 << 32)


def _expect_paillier(k):
    bits, p, q = k["bits"], k["p"], k["q"]
    assert p < q
    n = p * q
    ns = n * n
    L1 = 32 if bits <= 1024 else (64 if bits <= 2048 else 128)
    L2, LQ = 2 * L1, L1 // 2
    T2, Th, Ts = L2 // 32, L2 // 64, max(1, L2 // 128)
    R2 = 1 << (rad_lb(T2) * rad_ll(T2) * T2)  # R of the n^2 engine
    Rh = 1 << (rad_lb(Th) * rad_ll(Th) * Th)
    e = Expect()
    e.ctx = dict(L1=L1, L2=L2, LQ=LQ, has_sk=int(k["sk"]), kh_direct=int(k["sk"]), ou=0, ou_hwin=0, ou_tab=-1)
    e.words("N2", ns, L2)
    e.words("N2_R2", pow(2, 64 * L2, ns), L2)
    e.words("N2_R1", pow(2, 32 * L2, ns), L2)
    e.words("n", n, L1 + 1)
    e.words("nm1", n - 1, L1)
    e.words("max_int", n // 2, L1)
    e.words("n_mm", n - n // 2, L1)
    e.val.update(n2_n0inv=_inv32(ns), nbits=bits)
    e.modulus(ns, T2, "N2_27", "N2R1_27", "N2R2_27", "N2R3_27", "n2_np27")
    e.words("N2M1", R2 % ns, L2)
    e.modulus(n, Th, "Nn_27", "NnR1_27", "NnR2_27", None, "nn_np27")
    e.val["nn_inv27"] = pow(n, -1, 1 << rad_lb(Th))
    if not k["sk"]:
        return e
    ps, qs = p * p, q * q
    R32 = 1 << (32 * LQ)
    for s, t, s2, nm in ((p, q, ps, "p"), (q, p, qs, "q")):
        S = nm.upper()
        e.words(S + "2", s2, L1)
        e.words(S + "2_R3", pow(2, 96 * L1, s2), L1)
        e.words(nm + "m1", s - 1, LQ + 1)
        e.words(nm, s, LQ)
        e.words(nm + "inv2", pow(s, -1, R32), LQ)
        # h_s = L(g^(s-1) mod s^2)^-1 mod s, g = n + 1, L(x) = (x - 1) / s, as Montgomery residue
        # of the 32-bit CRT tail
        lval = (pow(n + 1, s - 1, s2) - 1) // s
        e.words(f"h{nm}R", pow(lval, -1, s) * R32 % s, LQ)
        e.modulus(s2, Th, S + "2_27", S + "2R1_27", S + "2R2_27", None, nm + "2_np27")
        e.limbs(S + "2RX_27", Rh * Rh * pow(R2, -1, s2) % s2, Th)
        e.val[nm + "2_n0inv"] = _inv32(s2)
        e.val[nm + "_n0inv"] = _inv32(s)
        e.val[nm + "m1_bits"] = (s - 1).bit_length()
        es = n % (s * (s - 1))
        e.words("e" + nm, es, L1)
        e.val[f"e{nm}_bits"] = es.bit_length()
        e.modulus(s, Ts, S + "s_27", None, S + "sR2_27", S + "sR3_27", nm + "s_np27")
        e1 = t % (s - 1)
        e.words("e1" + nm, e1, LQ)
        e.val[f"e1{nm}_bits"] = e1.bit_length()
        e.val[nm + "_bits"] = s.bit_length()
        t2 = t * t
        K = t2 * pow(t2, -1, s2)  # 1 mod s^2, 0 mod t^2
        assert K % s2 == 1 and K % t2 == 0
        e.limbs(f"K{nm}R_27", K * R2 % ns, T2)
    e.words("pinvqR", pow(p, -1, q) * R32 % q, LQ)
    assert (p - 1) % q and (q - 1) % p  # kh_direct
    return e


def _expect_ou(k):
    bits, n, g, h, p, q = k["bits"], k["n"], k["g"], k["h"], k["p"], k["q"]
    L2 = 64 if bits <= 2048 else 128
    L1 = L2 // 2
    T2 = L2 // 32
    lb, nl = rad_lb(T2), rad_ll(T2) * T2
    R = 1 << (lb * nl)
    e = Expect()
    e.words("N2", n, L2)
    e.words("n", n, L2 + 1)
    e.words("nm1", n - 1, L2)
    e.modulus(n, T2, "N2_27", "N2R1_27", "N2R2_27", "N2R3_27", "n2_np27")
    e.words("N2M1", R % n, L2)
    e.val.update(n2_n0inv=_inv32(n), nbits=bits, nn_inv27=pow(n, -1, 1 << lb))
    if p is not None:
        ps = p * p
        assert ps * q == n
        e.modulus(ps, T2, "P2_27", "P2R1_27", None, None, "p2_np27")
        e.words("pm1", p - 1, L1 + 1)
        e.words("p", p, L1)
        e.words("pinv2", pow(p, -1, 1 << (32 * L1)), L1)
        hp = pow((pow(g, p - 1, ps) - 1) // p, -1, p)
        e.words("hpR", hp * (1 << (32 * L1)) % p, L1)
        e.val.update(p_n0inv=_inv32(p), pm1_bits=(p - 1).bit_length(), p_bits=p.bit_length())
    hwin = (bits + OU_WIN - 1) // OU_WIN
    e.ctx = dict(L1=L1, L2=L2, LQ=L1 // 2, has_sk=int(p is not None), kh_direct=0, ou=1, ou_hwin=hwin)
    e.table = (hwin, L1 * 32 // OU_WIN, nl, lb, R)
    return e


@pytest.mark.parametrize("name", sorted(CASES))
def test_blob_constants(dumped, name):
    _, scheme, k = CASES[name]
    d = dumped[name]
    e = _expect_paillier(k) if scheme == "paillier" else _expect_ou(k)
    e.check(d, name)
    if scheme != "ou":
        return
    # the fixed-base table: row 0 = M(1), then M(h^(d 16^i)) for i < hwin, d = 1..15, then g's
    hwin, gwin, nl, lb, R = e.table
    n = k["n"]
    want = [R % n]
    for base, nwin in ((k["h"], hwin), (k["g"], gwin)):
        b = base % n
        for _ in range(nwin):
            x = b
            for _d in range(1, 1 << OU_WIN):
                want.append(x * R % n)
                x = x * b % n
            b = x  # base^(16^(i+1))
    # the walk above is itself pinned to pow at the far end of each base's windows
    assert want[-1] == pow(k["g"], 15 * 16 ** (gwin - 1), n) * R % n
    assert want[15 * hwin] == pow(k["h"], 15 * 16 ** (hwin - 1), n) * R % n
    tab = d["ctx"]["ou_tab"]
    assert tab >= 0 and tab % 64 == 0 and tab + len(want) * nl == d["blob"].size
    got = d["blob"][tab:].reshape(len(want), nl)
    bad = np.nonzero((got != _radix_rows(want, nl, lb)).any(axis=1))[0]
    assert bad.size == 0, (name, "table rows", bad[:8].tolist())


def test_every_fixture_key_is_dumped():
    """9 Paillier keys and the real OU key, public-only and with the secret key; 6 public OU moduli."""
    assert len(CASES) == 2 * 9 + 6 + 2
    for fam in ("ones", "ones_lo1", "sparse"):
        for bits in (1024, 2048, 4096):
            assert FX["paillier"][f"{fam}_{bits}"]["bits"] == bits
    for fam in ("allones", "ones_lo1", "sparse"):
        for bits in (2048, 4096):
            assert int(FX["ou_public"][f"{fam}_{bits}"]["n"], 16).bit_length() == bits
