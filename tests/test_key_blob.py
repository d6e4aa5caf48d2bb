"""The key blob and KeyArgs that context creation derives from a key, pinned for every committed
key (tests/golden/key_blob.json: the blob's length and SHA-256, every KeyArgs pointer as an offset
into it, every scalar, the context scalars).  The builder is plain C++ (fate_amd/csrc/key_blob.h,
no HIP header), so a stand-alone g++ program (tests/key_blob_dump.cpp) runs it here without a GPU;
fphe_ctx_create / fphe_ou_ctx_create call the same two functions.  Keys that are not keys keep
returning FPHE_ERR_KEY."""
import hashlib
import json
import os
import subprocess

import pytest

from tests import ou_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FPHE_OK, FPHE_ERR_KEY = 0, 4


def _paillier_keys():
    for name in ("paillier_1024.json", "paillier_2048.json", "key_4096.json"):
        with open(os.path.join(GOLDEN, name)) as f:
            fx = json.load(f)
        yield int(fx["p"], 16), int(fx["q"], 16)


def _line(name, scheme, bits, *ints):
    return " ".join([name, scheme, str(bits)] + ["-" if v is None else "%x" % v for v in ints])


def _cases():
    """(lines for the program, names expected to build, names expected to be rejected)"""
    lines, good, bad = [], [], []

    def add(ok, *a):
        lines.append(_line(*a))
        (good if ok else bad).append(a[0])

    for p, q in _paillier_keys():
        n, bits = p * q, (p * q).bit_length()
        add(True, f"paillier_{bits}_pk", "paillier", bits, n, None, None)
        add(True, f"paillier_{bits}_sk", "paillier", bits, n, p, q)
        if bits == 1024:
            add(False, "paillier_even_n", "paillier", bits, n + 1, None, None)
            add(False, "paillier_p_eq_q", "paillier", bits, n, p, p)
            add(False, "paillier_pq_ne_n", "paillier", bits, n + 2, p, q)
            add(False, "paillier_bits", "paillier", bits + 2, n, None, None)
    for bits, k in sorted(ou_ref.load_keys().items()):
        add(True, f"ou_{bits}_pk", "ou", bits, k.n, k.g, k.h, None, None)
        add(True, f"ou_{bits}_sk", "ou", bits, k.n, k.g, k.h, k.p, k.q)
        if bits == 1024:  # the cases of tests/test_gpu_ou.py::test_guards, and a g of order 1 mod p^2
            add(False, "ou_even_n", "ou", bits, k.n + 1, k.g, k.h, None, None)
            add(False, "ou_p_eq_q", "ou", bits, k.n, k.g, k.h, k.p, k.p)
            add(False, "ou_p2q_ne_n", "ou", bits, k.n + 2, k.g, k.h, k.p, k.q)
            add(False, "ou_g_zero", "ou", bits, k.n, 0, k.h, None, None)
            add(False, "ou_h_is_n", "ou", bits, k.n, k.g, k.n, None, None)
            add(False, "ou_bits", "ou", 1026, k.n, k.g, k.h, None, None)
            add(False, "ou_g_power_is_1", "ou", bits, k.n, 1, k.h, k.p, k.q)
    return lines, good, bad


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Build the program, run it once over every case: {name: status or the parsed dump}."""
    tmp = tmp_path_factory.mktemp("key_blob")
    exe = tmp / "key_blob_dump"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "key_blob_dump.cpp")], check=True)
    lines, _, _ = _cases()
    procs = []
    for i in range(4):  # the cases are independent: four processes, a quarter of the lines each
        (tmp / f"cases{i}.txt").write_text("\n".join(lines[i::4]) + "\n")
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
            cur["sha256"] = hashlib.sha256((tmp / (name + ".blob")).read_bytes()).hexdigest()
        else:
            cur[t[0]] = int(t[1])
    return out


def test_blobs_match_the_fixture(dumped):
    with open(os.path.join(GOLDEN, "key_blob.json")) as f:
        want = json.load(f)["cases"]
    _, good, _ = _cases()
    assert sorted(good) == sorted(want)
    for name in good:
        got = dict(dumped[name])
        assert got.pop("status") == FPHE_OK, name
        assert got == want[name], name


def test_rejected_keys_stay_rejected(dumped):
    _, _, bad = _cases()
    assert len(bad) == 11
    for name in bad:
        assert dumped[name] == {"status": FPHE_ERR_KEY, "ptr": {}, "val": {}, "ctx": {}}, name
