"""GPU edge cases of the hot path: empty and ragged vectors (partial 64-element tiles, a
single element, several waves), and a 2048-bit subset checked element by element against
libgmp (oracle/gmp_ref.c, the mpz_* call sequence rug issues for paillier/src/lib.rs:94-176).
Bit-exact on signed ciphertext integers, exponents and decoded float bits."""
import json
import os
import random

import numpy as np
import pytest
import torch

from fate_amd import paillier as P
from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def load(bits):
    with open(os.path.join(HERE, "golden", f"paillier_{bits}.json")) as f:
        fx = json.load(f)
    p, q = int(fx["p"], 16), int(fx["q"], 16)
    sk, pk, coder = P.keypair_from_primes(p, q)
    osk, opk = O.keypair_from_primes(p, q)
    return p, q, sk, pk, coder, osk, opk


@pytest.fixture(scope="module")
def k1024():
    return load(1024)


@pytest.mark.parametrize("n", [0, 1, 63, 65, 130])
def test_ragged_encrypt_add_mul_decrypt(k1024, n):
    """Sizes that are not whole tiles (and the empty vector) through every element-wise op."""
    p, q, sk, pk, coder, osk, opk = k1024
    rng = random.Random(100 + n)
    xs = [rng.uniform(-50, 50) for _ in range(n)]
    ys = [rng.uniform(-1e-3, 1e-3) for _ in range(n)]  # other exponents: exercises alignment
    ws = [rng.uniform(-2, 2) for _ in range(n)]
    rx = [1 + rng.randrange(opk.n - 1) for _ in range(n)]
    ry = [1 + rng.randrange(opk.n - 1) for _ in range(n)]
    xd = torch.tensor(xs, dtype=torch.float32).cuda()
    yd = torch.tensor(ys, dtype=torch.float32).cuda()
    wd = torch.tensor(ws, dtype=torch.float32).cuda()
    cx = pk.encrypt_encoded(coder.encode_f32_vec(xd), True, r=rx)
    cy = pk.encrypt_encoded(coder.encode_f32_vec(yd), True, r=ry)
    s = cx.add(pk, cy)
    m = cx.mul(pk, coder.encode_f32_vec(wd))
    dec = coder.decode_f32_vec(sk.decrypt_to_encoded(s)).cpu()
    assert len(cx) == n and len(s) == n and len(m) == n and dec.numel() == n
    xf = xd.cpu().tolist()
    yf = yd.cpu().tolist()
    wf = wd.cpu().tolist()
    ox = [O.fp_encrypt(opk, O.encode_f32(opk.n, v), True, r) for v, r in zip(xf, rx)]
    oy = [O.fp_encrypt(opk, O.encode_f32(opk.n, v), True, r) for v, r in zip(yf, ry)]
    osum = [O.ct_add(opk, a, b) for a, b in zip(ox, oy)]
    omul = [O.ct_mul(opk, a, O.encode_f32(opk.n, w)) for a, w in zip(ox, wf)]
    assert cx.to_signed_ints(pk.ns) == ([c.c for c in ox], [c.exp for c in ox])
    assert s.to_signed_ints(pk.ns) == ([c.c for c in osum], [c.exp for c in osum])
    assert m.to_signed_ints(pk.ns) == ([c.c for c in omul], [c.exp for c in omul])
    want = [float(O.decode_f32(opk.n, d.significant, d.exp)) for d in (O.fp_decrypt(osk, c) for c in osum)]
    assert np.array(dec.tolist(), dtype=np.float32).view(np.uint32).tolist() == \
        np.array(want, dtype=np.float32).view(np.uint32).tolist()


def test_gmp_subset_2048():
    """384 elements at 2048 bits (six waves of the encrypt kernel, a partial last tile)
    against libgmp: obfuscated encrypt with injected r, nude encrypt, CRT decrypt."""
    from oracle import gmp_ref
    p, q, sk, pk, coder, osk, opk = load(2048)
    gk = gmp_ref.GmpKey(p * q, p, q)
    n = 384 - 17
    rng = random.Random(2048)
    xs = torch.tensor([rng.gauss(0, 4) for _ in range(n)], dtype=torch.float32)
    pv = coder.encode_f32_vec(xs.cuda())
    sig, exp = pv.to_ints()
    r = [1 + rng.randrange(pk.n - 1) for _ in range(n)]
    ct = P.PK(pk.n).encrypt_encoded(pv, True, r=r)
    got, got_e = ct.to_signed_ints(pk.ns)
    assert got_e == exp
    assert got == [gk.encrypt(s, ri, True) for s, ri in zip(sig, r)]
    nude, _ = pk.encrypt_encoded(pv, False).to_signed_ints(pk.ns)
    assert nude == [gk.encrypt(s, None, False) for s in sig]
    dsig, dexp = sk.decrypt_to_encoded(ct).to_ints()
    assert dexp == exp
    assert dsig == [gk.decrypt(c) for c in got]
    assert dsig == [s % pk.n for s in sig]


def test_permute_gather_assign_cat():
    """fphe_permute (gather / scatter of tile-major vectors) against torch indexing, and the
    vector plumbing built on it: _assign, slice_indexes (with the reference's out-of-range
    panic), cat of vectors that are not whole tiles."""
    g = torch.Generator().manual_seed(3)
    t = torch.randint(0, 2**31 - 1, (5, 7, 64), dtype=torch.int32, generator=g).cuda()
    sg = torch.randint(0, 2, (320,), dtype=torch.uint8, generator=g).cuda()
    ex = torch.randint(-20, 20, (320,), dtype=torch.int32, generator=g).cuda()
    v = P.CiphertextVector(t.clone(), sg.clone(), ex.clone(), 317)
    idx = torch.tensor([3, 200, 64, 0, 316, 5, 5, 130])
    got = v._gather(idx)
    cols = P.tiles_to_cols(t.cpu())
    assert got.count == 8 and got.C.shape == (1, 7, 64)
    assert torch.equal(P.tiles_to_cols(got.C.cpu())[:, :8], cols[:, idx])
    assert torch.equal(P.tiles_to_cols(got.C.cpu())[:, 8:], torch.zeros(7, 56, dtype=torch.int32))
    assert got.sign[:8].cpu().tolist() == sg.cpu()[idx].tolist() and got.exp[:8].cpu().tolist() == ex.cpu()[idx].tolist()
    w = P.CiphertextVector(t.clone(), sg.clone(), ex.clone(), 317)
    dst = torch.tensor([10, 11, 300, 12, 64, 1, 2, 3])
    w._assign(dst, got)
    wc = P.tiles_to_cols(w.C.cpu())
    assert torch.equal(wc[:, dst], cols[:, idx])
    untouched = torch.tensor([i for i in range(317) if i not in set(dst.tolist())])
    assert torch.equal(wc[:, untouched], cols[:, untouched])
    assert w.sign.cpu()[dst].tolist() == sg.cpu()[idx].tolist() and w.exp.cpu()[dst].tolist() == ex.cpu()[idx].tolist()
    s2 = v.slice_indexes([316, 0, 7])
    assert torch.equal(P.tiles_to_cols(s2.C.cpu())[:, :3], cols[:, [316, 0, 7]])
    with pytest.raises(P.PanicException):
        v.slice_indexes([0, 317])
    a = P.CiphertextVector(t[:2].clone(), sg[:128].clone(), ex[:128].clone(), 100)
    b = P.CiphertextVector(t[2:4].clone(), sg[128:256].clone(), ex[128:256].clone(), 70)
    c = P.Evaluator.cat([a, b])
    cc = P.tiles_to_cols(c.C.cpu())
    assert c.count == 170
    assert torch.equal(cc[:, :100], cols[:, :100]) and torch.equal(cc[:, 100:170], cols[:, 128:198])
    assert c.exp[:170].cpu().tolist() == ex.cpu()[:100].tolist() + ex.cpu()[128:198].tolist()



@pytest.mark.parametrize("bits", [1024, 3072])
def test_add_gap_sorted_matches_kernel_order(k1024, bits):
    """fphe_add over the device launch order (fate_amd.paillier._add_order: XCD runs, gap
    bins) gives the same ciphertexts as the kernel in element order; decrypted sums match the
    floats.  3072 bits: k_add27 on the TPI-8 geometry (8 elements per wave tile)."""
    if bits == 1024:
        p, q, sk, pk, coder, osk, opk = k1024
    else:
        sk, pk, coder = P.keygen(bits)
    n = 8192 + 33
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 12, (n,), generator=g).float())
    y = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 12, (n,), generator=g).float())
    cx = pk.encrypt_encoded(coder.encode_f32_vec(x.cuda()), True)
    cy = pk.encrypt_encoded(coder.encode_f32_vec(y.cuda()), True)
    assert P._add_order(cx.exp[:n], cy.exp[:n], cx.L2) is not None  # the sorted path runs
    s_sorted = P._add(pk, cx, cy, False)
    s_plain = P._add(pk, cx, cy, False, reorder=False)
    assert s_sorted.to_signed_ints(pk.ns) == s_plain.to_signed_ints(pk.ns)
    d = coder.decode_f64_vec(sk.decrypt_to_encoded(s_sorted)).cpu()
    assert torch.allclose(d, x.double() + y.double(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("m,L2", [(1, 128), (4097, 128), (70000, 64), (300001, 128), (1 << 20, 256)])
def test_add_order_device_counting_sort(m, L2):
    """fphe_add_order (the ct-add launch order) against its contract: a permutation; run r
    (ceil(wave tiles / 8) tiles) holds exactly its own element range; inside a run the gaps
    >= 3 come first in non-increasing order, then every 4096-element block's elements
    contiguously, non-increasing gaps within the block."""
    g = torch.Generator().manual_seed(m)
    eb = torch.randint(-40, 40, (m,), generator=g, dtype=torch.int32)
    d = torch.multinomial(torch.tensor([0.37, 0.55, 0.05, 0.02, 0.01]), m, replacement=True, generator=g)
    d = d.to(torch.int32) * torch.where(torch.rand(m, generator=g) < 0.001, 20, 1).to(torch.int32)
    ea = eb + d * torch.where(torch.rand(m, generator=g) < 0.5, 1, -1).to(torch.int32)
    o = P._add_order(ea.cuda(), eb.cuda(), L2).cpu().long()
    assert torch.equal(torch.sort(o)[0], torch.arange(m))
    E = 64 // (L2 // 32)
    nwt = (m + E - 1) // E
    run = (nwt + 7) // 8 * E
    gap = (ea - eb).abs().clamp(max=63)
    for r in range(8):
        lo, hi = r * run, min((r + 1) * run, m)
        if lo >= hi:
            continue
        seg = o[lo:hi]
        assert int(seg.min()) >= lo and int(seg.max()) < hi
        gs = gap[seg]
        nh = int((gs >= 3).sum())
        assert bool((gs[:nh] >= 3).all()) and bool((gs[nh:] < 3).all())
        assert bool((gs[:nh][1:] <= gs[:nh][:-1]).all())
        light, lg = seg[nh:], gs[nh:]
        blk = (light - lo) // 4096
        assert bool((blk[1:] >= blk[:-1]).all())  # blocks in order, each contiguous
        same = blk[1:] == blk[:-1]
        assert bool((lg[1:][same] <= lg[:-1][same]).all())


@pytest.mark.parametrize("bits", [1024, 2048])
def test_export_import_signed(bits):
    """fphe_export_signed / fphe_import_signed against the host conversion of the fixtures'
    signed reference integers (negative ciphertexts included)."""
    p, q, sk, pk, coder, osk, opk = load(bits)
    with open(os.path.join(HERE, "golden", f"paillier_{bits}.json")) as f:
        fx = json.load(f)
    cs = [int(c, 16) for c in fx["encrypt"]["ct"]] + [1, -1]
    es = fx["encrypt"]["exp"] + [0, 3]
    v = P.CiphertextVector.from_signed_ints(cs, es, pk.ns, pk._key.L2)
    assert any(c < 0 for c in cs)
    mag, neg, ex = v.export_signed(pk)
    m = mag.cpu().numpy().view(np.uint32)
    got = [(-1 if int(ng) else 1) * sum(int(w) << (32 * k) for k, w in enumerate(row))
           for row, ng in zip(m, neg.cpu().tolist())]
    assert got == cs and ex.cpu().tolist() == es
    back = P.CiphertextVector.import_signed(pk, mag, neg, ex)
    assert back.to_signed_ints(pk.ns) == (cs, es)


def test_two_streams_share_a_context(k1024):
    """Encryptions issued on two HIP streams with one key context: the context's scratch
    (window tables) is handed from one stream to the other only after the first finishes,
    so both results decrypt exactly."""
    p, q, sk, pk, coder, osk, opk = k1024
    g = torch.Generator().manual_seed(17)
    xa = (torch.randn(4096, generator=g) * 8).cuda()
    xb = (torch.randn(6000, generator=g) * 8).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ca = pk.encrypt_encoded(coder.encode_f32_vec(xa), True)
    with torch.cuda.stream(s2):
        cb = pk.encrypt_encoded(coder.encode_f32_vec(xb), True)
    torch.cuda.synchronize()
    for x, c in ((xa, ca), (xb, cb)):
        y = coder.decode_f32_vec(sk.decrypt_to_encoded(c))
        assert torch.equal(y.cpu().view(torch.int32), x.cpu().view(torch.int32))


def test_two_threads_share_a_context(k1024):
    """Two host threads, each on its own HIP stream, run encrypt -> ct-add -> ct x pt ->
    decrypt loops with one key context at once (the context's lock orders the launches and
    its scratch hand-over between streams): every result decodes to the float64 value of the
    same ops."""
    import threading
    p, q, sk, pk, coder, osk, opk = k1024
    errors = []

    def work(seed, n):
        try:
            g = torch.Generator().manual_seed(seed)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    x = torch.randint(-1000, 1000, (n,), generator=g).double().cuda()
                    y = torch.randint(-1000, 1000, (n,), generator=g).double().cuda()
                    w = torch.randint(-9, 9, (n,), generator=g).double().cuda()
                    cx = pk.encrypt_encoded(coder.encode_f64_vec(x), True)
                    cy = pk.encrypt_encoded(coder.encode_f64_vec(y), True)
                    r = cx.add(pk, cy).mul(pk, coder.encode_f64_vec(w))
                    got = coder.decode_f64_vec(sk.decrypt_to_encoded(r))
                    s.synchronize()
                    if not torch.equal(got, (x + y) * w):
                        errors.append(seed)
        except Exception as e:  # surfaced below
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(seed, n)) for seed, n in ((1, 300), (2, 5000))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("bits,seed", [(1024, 0), (1024, 1), (1024, 2), (2048, 0), (2048, 1)])
def test_random_op_chains_vs_oracle(bits, seed):
    """Randomised chains of the element-wise ops (add / sub / rsub / add_pt / ct x pt with
    float, negative-float and encoded-negative-integer plaintexts / neg / i_double) over
    vectors of random ragged length, every intermediate compared bit-exact with the oracle
    (fixedpoint_paillier/src/lib.rs:250-349), at 1024 and 2048 bits (the starting encryptions
    by libgmp, oracle/gmp_ref.c, which the oracle's own encrypt is pinned to)."""
    import random as _r
    from oracle import gmp_ref
    p, q, sk, pk, coder, osk, opk = load(bits)
    gk = gmp_ref.GmpKey(p * q, p, q)
    rng = _r.Random(1000 + seed + bits)
    n = rng.randrange(1, 200)

    def rand_pt():
        k = rng.randrange(4)
        if k == 0:
            return O.encode_f64(opk.n, rng.uniform(-1e3, 1e3))
        if k == 1:
            return O.encode_f64(opk.n, rng.uniform(-1e-6, 1e-6))
        if k == 2:
            return O.encode_i64(opk.n, rng.randrange(-(1 << 40), 1 << 40))
        return O.encode_f64(opk.n, float(rng.randrange(-5, 5)))

    def dev_pts(pts):
        return P.PlaintextVector.from_ints([x.significant for x in pts], [x.exp for x in pts])

    def enc(pt):
        return O.Ciphertext(gk.encrypt(pt.significant, 1 + rng.randrange(opk.n - 1), True), pt.exp)

    oa = [enc(rand_pt()) for _ in range(n)]
    ob = [enc(rand_pt()) for _ in range(n)]
    da = P.CiphertextVector.from_signed_ints([c.c for c in oa], [c.exp for c in oa], pk.ns, pk._key.L2)
    db = P.CiphertextVector.from_signed_ints([c.c for c in ob], [c.exp for c in ob], pk.ns, pk._key.L2)
    for _ in range(6):
        op = rng.choice(["add", "sub", "rsub", "add_pt", "mul", "neg", "double"])
        if op == "add":
            oa, da = [O.ct_add(opk, x, y) for x, y in zip(oa, ob)], da.add(pk, db)
        elif op == "sub":
            oa, da = [O.ct_sub(opk, x, y) for x, y in zip(oa, ob)], da.sub(pk, db)
        elif op == "rsub":
            oa, da = [O.ct_rsub(opk, x, y) for x, y in zip(oa, ob)], da.rsub(pk, db)
        elif op == "add_pt":
            pts = [rand_pt() for _ in range(n)]
            enc = pk.encrypt_encoded(dev_pts(pts), False)
            oa, da = [O.ct_add_pt(opk, x, y) for x, y in zip(oa, pts)], da.add(pk, enc)
        elif op == "mul":
            pts = [rand_pt() for _ in range(n)]
            oa, da = [O.ct_mul(opk, x, y) for x, y in zip(oa, pts)], da.mul(pk, dev_pts(pts))
        elif op == "neg":
            oa, da = [O.ct_neg(opk, x) for x in oa], da.neg(pk)
        else:
            oa = [O.ct_add(opk, x, x) for x in oa]
            da = da.add(pk, da)
        assert da.to_signed_ints(pk.ns) == ([c.c for c in oa], [c.exp for c in oa]), op
    got = coder.decode_f64_vec(sk.decrypt_to_encoded(da)).cpu().tolist()
    want = [O.decode_f64(opk.n, d.significant, d.exp) for d in (O.fp_decrypt(osk, c) for c in oa)]
    assert [float(x) for x in got] == [float(x) for x in want]


@pytest.mark.parametrize("bits", [256, 258, 512, 770, 1026, 1030, 1536, 2050, 3072, 4096])
def test_other_key_sizes_bit_exact(bits):
    """Even key sizes other than 1024 / 2048 (the reference takes any even size, paillier/
    src/lib.rs:72-87; he_param.key_length is a job parameter) run the 1024-, 2048- or 4096-bit
    kernels with n zero-padded (above 2048 bits n^2 spans 8 lanes per element, TPI 8):
    encrypt (public and key-holder, injected r), ct-add with exponent alignment, ct x pt with
    negative weights, neg and decrypt, bit-exact against the oracle on a freshly generated
    key, and the public-key encryptions against libgmp."""
    import random
    from oracle import gmp_ref
    sk, pk, coder = P.keygen(bits)
    assert pk.n.bit_length() == bits
    osk, opk = O.keypair_from_primes(sk.p, sk.q)
    rng = random.Random(bits)
    nx = 70 if bits <= 2048 else 40  # the Python oracle's powm at 8192 bits is the slow side
    xs = [rng.uniform(-9, 9) for _ in range(nx)] + [0.0, -1e-300, 3e38]
    ws = [rng.uniform(-2, 2) for _ in xs]
    rs = [1 + rng.randrange(pk.n - 1) for _ in xs]
    xd = torch.tensor(xs, dtype=torch.float64, device="cuda")
    pv = coder.encode_f64_vec(xd)
    pub = P.PK(pk.n)
    c = pub.encrypt_encoded(pv, True, r=rs)
    ck = pk.encrypt_encoded(pv, True, r=rs)  # key-holder CRT path
    oc = [O.fp_encrypt(opk, O.encode_f64(opk.n, x), True, r) for x, r in zip(xs, rs)]
    want = ([o.c for o in oc], [o.exp for o in oc])
    assert c.to_signed_ints(pk.ns) == want and ck.to_signed_ints(pk.ns) == want
    gk = gmp_ref.GmpKey(pk.n, sk.p, sk.q)
    sig, _ = pv.to_ints()
    assert want[0] == [gk.encrypt(s_, r, True) for s_, r in zip(sig, rs)]
    y = pub.encrypt_encoded(coder.encode_f64_vec(xd.flip(0) * 1e-3), True, r=rs[::-1])
    oy = [O.fp_encrypt(opk, O.encode_f64(opk.n, x * 1e-3), True, r) for x, r in zip(xs[::-1], rs[::-1])]
    s = c.add(pk, y)
    assert s.to_signed_ints(pk.ns) == ([t.c for t in O.vec_add(opk, oc, oy)], [t.exp for t in O.vec_add(opk, oc, oy)])
    m = c.mul(pk, coder.encode_f64_vec(torch.tensor(ws, dtype=torch.float64, device="cuda")))
    om = [O.ct_mul(opk, a, O.encode_f64(opk.n, w)) for a, w in zip(oc, ws)]
    assert m.to_signed_ints(pk.ns) == ([t.c for t in om], [t.exp for t in om])
    ng = c.neg(pk)
    assert ng.to_signed_ints(pk.ns)[0] == [O.ct_neg(opk, a).c for a in oc]
    dec = sk.decrypt_to_encoded(s).to_ints()
    od = [O.fp_decrypt(osk, t) for t in O.vec_add(opk, oc, oy)]
    assert dec == ([d.significant for d in od], [d.exp for d in od])
    # pack_squeeze on the one-chunk-per-wave kernel at this geometry (wide_dev.h)
    sq = c.pack_squeeze(3, 61, pk)
    osq = O.pack_squeeze(opk, oc, 3, 61)
    assert sq.to_signed_ints(pk.ns) == ([t.c for t in osq], [t.exp for t in osq])
    # the key holder's device-drawn obfuscation ((z_p, z_q), k_draw_z) at this geometry: few
    # elements (k_pow_half_enc_wide) and past the latency threshold (k_pow_half27<., ., true,
    # true>) decrypt to the inputs, and the obfuscation is an n-th residue (x^lambda = 1 mod n^2)
    lam = (sk.p - 1) * (sk.q - 1)
    kd = pk.encrypt_encoded(pv, True)
    assert coder.decode_f64_vec(sk.decrypt_to_encoded(kd)).cpu().tolist() == xs
    cs, _ = kd.to_signed_ints(pk.ns)
    for cc, s_ in list(zip(cs, sig))[:3]:
        xo = (cc % pk.ns) * pow((1 + (s_ % pk.n) * pk.n) % pk.ns, -1, pk.ns) % pk.ns
        assert pow(xo, lam, pk.ns) == 1
    xb = torch.randn(4100, generator=torch.Generator().manual_seed(bits), dtype=torch.float64, device="cpu").cuda()
    kb = pk.encrypt_encoded(coder.encode_f64_vec(xb), True)
    assert torch.equal(coder.decode_f64_vec(sk.decrypt_to_encoded(kb)), xb)


def test_unsupported_key_sizes_decline():
    """Sizes this backend does not run fail at keygen with ValueError (FATE keeps its CPU
    path for them); odd sizes fail like the reference's assert."""
    from fate_amd import protocol as PR
    assert PR.supports(2048) and PR.supports(1536) and PR.supports(3072) and PR.supports(4096)
    assert not PR.supports(4098) and not PR.supports(1023) and not PR.supports(254)
    with pytest.raises(ValueError):
        PR.keygen(4098)
    with pytest.raises(AssertionError):
        P.keygen(1023)


def run_extreme_operands(p, q, count=None):
    """The body of test_extreme_operands for the key (p, q); tests/test_gpu_extreme_moduli.py runs
    it on the keys whose moduli are themselves extreme.  The operands are the canonical edge values
    below and, so that all-ones limbs reach the kernels as such, the canonical values whose
    resident form M(c) = c R mod n^2 is an edge pattern (tests/extreme_ref.py; the canonical
    n^2 - 1 is stored as a random-looking M(.)).  count: keep that many operands (the widest
    keys, where the Python reference is the slow side), resident patterns first."""
    from tests import extreme_ref as X
    sk, pk, coder = P.keypair_from_primes(p, q)
    osk, opk = O.keypair_from_primes(p, q)
    ns, n = opk.ns, opk.n
    L = ns.bit_length()
    m28 = (L - 1) // 28
    vals = [2, ns - 1, ns - 2, (ns - 1) // 2, (1 << (L - 1)) - 1, (1 << (28 * m28)) - 1,
            ns - (1 << (28 * (m28 - 1))), int("5" * (L // 4 - 1), 16) % ns, 1]
    base = len(vals)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = X.resident_patterns(ns, pk._key.L2)
    extra = X.units(X.canonical(res, X.mont_r(pk._key, dev), ns), ns)  # neg below needs units
    assert len(extra) == len(res)  # a pattern is a multiple of p or q for no committed key
    vals = vals + extra
    if count is not None:
        vals = (extra + vals[:base])[:count]
    nv = len(vals)

    def cyc(xs):
        return [xs[i % len(xs)] for i in range(nv)]

    signs = cyc([0, 1, 0, 1, 0, 0, 1, 0, 0])
    cts = [O.Ciphertext(-(ns - v) if s else v, e) for v, s, e in zip(vals, signs, cyc([0, -3, 2, 0, -1, 0, 5, -2, 0]))]
    other = [O.Ciphertext(v, e) for v, e in zip(reversed(vals), cyc([1, 0, -3, 4, 0, -1, 0, 0, 3]))]
    dv = P.CiphertextVector.from_signed_ints([c.c for c in cts], [c.exp for c in cts], pk.ns, pk._key.L2)
    dw = P.CiphertextVector.from_signed_ints([c.c for c in other], [c.exp for c in other], pk.ns, pk._key.L2)
    # the resident patterns arrive on the device as listed
    if count is None:
        rows = P.tiles_to_cols(dv.C).t()[base:nv].cpu().numpy().view(np.uint32)
        stored = [sum(int(w) << (32 * k) for k, w in enumerate(r)) for r in rows]
        assert all(s_ in res for s_ in stored) and len(set(stored)) == len(extra)

    def host(v):
        cs, es = v.to_signed_ints(pk.ns)
        return list(zip(cs, es))

    assert host(dv) == [(c.c, c.exp) for c in cts]
    assert host(dv.add(pk, dw)) == [(c.c, c.exp) for c in (O.ct_add(opk, a, b) for a, b in zip(cts, other))]
    assert host(dv.neg(pk)) == [(c.c, c.exp) for c in (O.ct_neg(opk, a) for a in cts)]
    pts = [O.Plaintext(v, e) for v, e in zip(cyc([3, n - 5, n - 1, n // 2, 1, 0, 7, (1 << 60) + 1, 2]),
                                             cyc([0, 0, 1, -1, 0, 0, 0, -2, 0]))]
    pv = P.PlaintextVector.from_ints([t.significant for t in pts], [t.exp for t in pts])
    assert host(dv.mul(pk, pv)) == [(c.c, c.exp) for c in (O.ct_mul(opk, a, t) for a, t in zip(cts, pts))]
    gaps = cyc([5, 0, 1, 31, 2, 0, 3, 9, 4])
    al = P._align(pk, dv, torch.tensor(gaps))
    assert host(al) == [((c.c if g == 0 else pow(c.c % ns, 16 ** g, ns)), c.exp) for c, g in zip(cts, gaps)]
    sig, _ = sk.decrypt_to_encoded(dv).to_ints()
    assert sig == [O.decrypt(osk, c.c) for c in cts]
    # obfuscated encryption at the significand edges with r = 1 and r = n - 1 (a significand
    # above n/4 takes the reference's invert branch)
    maxi = n // 2
    sigs = [maxi, -maxi, 1, -1, 0, maxi - 1, n // 4, n // 4 + 1]
    rs = [1, n - 1, n - 1, 1, n - 1, 2, 1, n - 1]
    want = [O.fp_encrypt(opk, O.Plaintext(sg, 0), True, r) for sg, r in zip(sigs, rs)]
    pk_pub = P.keypair_from_primes(p, q, keyholder=False)[1]
    for k in (pk, pk_pub):  # key-holder CRT path and public-key path
        enc = k.encrypt_encoded(P.PlaintextVector.from_ints(sigs, [0] * len(sigs)), True, r=rs)
        assert host(enc) == [(c.c, c.exp) for c in want]


@pytest.mark.parametrize("bits", [1024, 2048])
def test_extreme_operands(bits):
    """Operands at the edges of the 28-bit engine's bounds (all-ones limbs, n^2 - 1, 2^k - 1
    just under n^2, 2, the literal 1, and the values whose resident form is all-ones limbs, one
    limb zero at a lane seam, alternating limbs) through ct-add with exponent gaps, ct x pt by
    small, big (n - small: a full-size exponent) and negative plaintexts, neg, the exponent
    alignment and decrypt; obfuscated encryption with r = 1 and r = n - 1 of the largest and
    smallest encodable significands.  Bit-exact against the oracle."""
    p, q = load(bits)[:2]
    run_extreme_operands(p, q)


def _rows(v, idx, pk):
    """The reference's (signed integer, exp) of elements idx of a device vector, read without
    a full copy (the elements are gathered, then exported out of the Montgomery form)."""
    idx_t = torch.as_tensor(idx, dtype=torch.long, device=v.C.device)
    return v._gather(idx_t).to_signed_ints(pk.ns)


def test_add_across_launch_chunks():
    """ct-add over vectors larger than one fphe_add_ordered launch (paillier.ADD_CHUNK
    elements, 2 GiB of ciphertext words at 2048 bits): the chunks' gap orders, tile offsets
    and ragged last tile, checked element by element against the oracle at the chunk seams,
    the ends and random positions (fixedpoint_paillier/src/lib.rs:301-333)."""
    p, q, sk, pk, coder, osk, opk = load(2048)
    n = P.ADD_CHUNK + 3 * 64 + 5
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    L2 = pk._key.L2

    def rand_vec():
        v = P.CiphertextVector.empty(n, L2, dev)
        v.C.copy_(torch.randint(-(1 << 31), 1 << 31, v.C.shape, generator=g, device=dev, dtype=torch.int32))
        v.C[:, L2 - 1, :] = 0  # < 2^(32(L2-1)) < n^2: canonical residues
        v.sign.copy_(torch.randint(0, 2, v.sign.shape, generator=g, device=dev, dtype=torch.uint8))
        v.exp.copy_(torch.randint(-16, -11, v.exp.shape, generator=g, device=dev, dtype=torch.int32))
        v.n = pk.n
        return v

    a, b = rand_vec(), rand_vec()
    seam = P.ADD_CHUNK
    lits = [0, seam - 1, seam, n - 1]
    one = pk._key.mont_one(dev)  # the literal 1 as stored: M(1)
    for i in lits[:2]:  # literal 1s on both sides of the seam
        a.C[i // 64, :, i % 64] = one
        a.sign[i] = 0
    for i in lits[2:]:
        b.C[i // 64, :, i % 64] = one
        b.sign[i] = 0
    out = a.add(pk, b)
    rng = random.Random(9)
    idx = sorted(set(lits + [1, 63, 64, seam - 64, seam - 2, seam + 1, seam + 63, seam + 64, n - 2, n - 64]
                     + [rng.randrange(n) for _ in range(24)]))
    (ca, ea), (cb, eb), (co, eo) = _rows(a, idx, pk), _rows(b, idx, pk), _rows(out, idx, pk)
    for k in lits:
        assert ca[idx.index(k)] == 1 or cb[idx.index(k)] == 1, k  # M(1) is the integer 1
    for k in range(len(idx)):
        want = O.ct_add(opk, O.Ciphertext(ca[k], ea[k]), O.Ciphertext(cb[k], eb[k]))
        assert (co[k], eo[k]) == (want.c, want.exp), idx[k]


@pytest.mark.parametrize("keyholder", [False, True], ids=["public", "keyholder_crt"])
def test_spans_match_one_launch(monkeypatch, keyholder):
    """Long encrypt / decrypt calls run as spans of whole grid rounds (fate_phe.hip
    span_elems): forced down to one round per span, a call over several spans gives the same
    ciphertexts as one launch -- device-drawn nonces included (each element draws the stream
    of its index in the call) -- and decrypts to the same plaintexts."""
    p, q, sk, pk, coder, osk, opk = load(1024)
    if not keyholder:
        pk = P.PK(pk.n)
    assert pk.keyholder == keyholder
    key = pk._priv if keyholder else pk._key
    n = 250_000 + 37  # > 2 one-round spans at 1024 bits (98,304 or 196,608 elements)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n, generator=g) * 4).cuda()
    x[-1000:] = x[:1000]  # the same plaintexts in the first and the last span
    pv = coder.encode_f32_vec(x)
    monkeypatch.setattr(key, "next_nonce", lambda: 4242)
    rng = random.Random(17)
    rs = [1 + rng.randrange(pk.n - 1) for _ in range(n)]  # injected nonces (parity mode)
    one = pk.encrypt_encoded(pv, True)
    d_one = sk.decrypt_to_encoded(one)
    one_r = pk.encrypt_encoded(pv, True, r=rs)
    monkeypatch.setenv("FPHE_SPAN_TARGET", "1")
    spans = pk.encrypt_encoded(pv, True)
    d_spans = sk.decrypt_to_encoded(spans)
    spans_r = pk.encrypt_encoded(pv, True, r=rs)
    monkeypatch.delenv("FPHE_SPAN_TARGET")
    assert torch.equal(P.tiles_to_cols(one_r.C)[:, :n], P.tiles_to_cols(spans_r.C)[:, :n])
    # elements past the count (the last tile's padding lanes) hold unspecified words
    assert torch.equal(P.tiles_to_cols(one.C)[:, :n], P.tiles_to_cols(spans.C)[:, :n])
    assert torch.equal(one.sign[:n], spans.sign[:n])
    assert torch.equal(P.tiles_to_cols(d_one.P)[:, :n], P.tiles_to_cols(d_spans.P)[:, :n])
    y = coder.decode_f32_vec(d_spans).cpu().numpy().view(np.uint32)
    xb = x.cpu().numpy().view(np.uint32)
    assert (y == np.where(xb == 0x80000000, 0, xb)).all()
    # no nonce stream repeats across spans: equal plaintexts, different ciphertexts
    assert not torch.equal(spans.C[:15], spans.C[(n - 1000) // 64:(n - 1000) // 64 + 15])
    cs = P.tiles_to_cols(spans.C.cpu())
    assert not any(torch.equal(cs[:, i], cs[:, n - 1000 + i]) for i in range(64))


def test_mul_spans_match_one_launch(monkeypatch):
    """ct x pt split into spans (forced to one grid round each) equals one launch: per-element
    plaintexts with negative weights (the batch inverse per span) and a broadcast scalar."""
    p, q, sk, pk, coder, osk, opk = load(1024)
    n = 300_000 + 11
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(n, generator=g) * 4).cuda()
    w = (torch.rand(n, generator=g) * 3 - 1).cuda()  # a third negative
    ct = pk.encrypt_encoded(coder.encode_f32_vec(x), True)
    pw = coder.encode_f32_vec(w)
    sc = P.Plaintext(coder.encode_f32_vec(torch.tensor([-1.25], device="cuda")))
    one, one_s = ct.mul(pk, pw), ct.mul_scalar(pk, sc)
    monkeypatch.setenv("FPHE_SPAN_TARGET", "1")
    sp, sp_s = ct.mul(pk, pw), ct.mul_scalar(pk, sc)
    monkeypatch.delenv("FPHE_SPAN_TARGET")
    for a, b in ((one, sp), (one_s, sp_s)):
        assert torch.equal(P.tiles_to_cols(a.C)[:, :n], P.tiles_to_cols(b.C)[:, :n])
        assert torch.equal(a.sign[:n], b.sign[:n]) and torch.equal(a.exp[:n], b.exp[:n])
    d = coder.decode_f64_vec(sk.decrypt_to_encoded(sp)).cpu()
    assert torch.allclose(d, (x.double() * w.double()).cpu(), rtol=1e-6, atol=1e-6)


def test_config2_subset_4096_vs_gmp(kernel_path):
    """SURVEY.md §8(d) config 2's bit-exact subset at full size: the first 4,096 elements of the
    bench's 1M float32 tensor (randn * 4, seed 20241218, the edge values up front) at 2048
    bits, with injected obfuscation nonces: the public-key encrypt, the key-holder (CRT)
    encrypt and the CRT decrypt against libgmp (oracle/gmp_ref.c: the mpz_* sequence rug issues
    for paillier/src/lib.rs:94-176, in 16 worker processes), and the decoded float32 bits
    against the inputs (-0.0 decodes as +0.0, as the reference's zero significand does)."""
    from oracle import gmp_ref
    p, q, sk, pk, coder, osk, opk = load(2048)
    g = torch.Generator().manual_seed(20241218)
    x = torch.randn(1 << 20, generator=g, dtype=torch.float32) * 4
    x[:8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3.4e38, -3.4e38, 1.0, -1.0])
    x = x[:4096].contiguous()
    pv = coder.encode_f32_vec(x.cuda())
    sig, exp = pv.to_ints()
    assert [(e.significant, e.exp) for e in (O.encode_f32(opk.n, v) for v in x.tolist())] == list(zip(sig, exp))
    rng = np.random.default_rng(4096)
    r = [1 + int.from_bytes(rng.bytes(256), "little") % (pk.n - 1) for _ in range(4096)]
    want = gmp_ref.parallel("encrypt", p * q, p, q, list(zip(sig, r)))
    got, got_e = P.PK(pk.n).encrypt_encoded(pv, True, r=r).to_signed_ints(pk.ns)
    assert got_e == exp and got == want
    ck = pk.encrypt_encoded(pv, True, r=r)  # the key holder's CRT path: the same integers
    assert ck.to_signed_ints(pk.ns)[0] == want
    dsig, dexp = sk.decrypt_to_encoded(ck).to_ints()
    assert dexp == exp and dsig == gmp_ref.parallel("decrypt", p * q, p, q, want)
    bits = coder.decode_f32_vec(sk.decrypt_to_encoded(ck)).cpu().view(torch.int32)
    xb = x.view(torch.int32).clone()
    xb[xb == -2147483648] = 0  # -0.0
    assert torch.equal(bits, xb)


@pytest.mark.parametrize("bits", [3072])
def test_large_key_vector_ops_and_pickle(bits, monkeypatch):
    """The 4096-bit geometry (TPI 8) through the vector ops above the element-wise kernels:
    the device-grouped fold under iupdate (terms with several exponents, negative signed
    ciphertexts, literal 1s), cumsum, and the reference's pickle state (bincode of the signed
    integers, paillier.rs:219-226) of an L2 = 256 vector, against the oracle's sequential
    Ciphertext::add (fixedpoint_paillier/src/lib.rs:301-333, 724-771)."""
    import pickle
    import random
    from fate_amd import wire
    sk, pk, coder = P.keygen(bits)
    osk, opk = O.keypair_from_primes(sk.p, sk.q)
    assert pk._key.L2 == 256
    rng = random.Random(bits + 1)
    src = []
    for i in range(150):
        r = rng.random()
        if r < 0.05:
            src.append(O.Ciphertext(1, rng.choice([0, -14])))
        else:
            c = rng.randrange(2, opk.ns)
            src.append(O.Ciphertext(-c if rng.random() < 0.3 else c, rng.choice([-14, -13, -13, -12, -15])))
    dv = P.CiphertextVector.from_signed_ints([c.c for c in src], [c.exp for c in src], pk.ns, pk._key.L2)
    # iupdate: 75 samples x (2 positions) x stride 2 into 10 x 2 slots
    nslot = 10
    positions = [[rng.randrange(nslot), rng.randrange(nslot)] for _ in range(75)]
    hist = P.CiphertextVector.zeros(nslot * 2, pk._key.L2)
    hist.iupdate(dv, positions, 2, pk)
    want = [O.ct_zero() for _ in range(nslot * 2)]
    O.iupdate(opk, want, src, positions, 2)
    assert hist.to_signed_ints(pk.ns) == ([c.c for c in want], [c.exp for c in want])
    # the same fold with every key above its slot's least exponent raised inside k_segfold27
    # (the slot plan on the TPI-8 geometry)
    monkeypatch.setenv("FPHE_FOLD_RAISE", "force")
    hist2 = P.CiphertextVector.zeros(nslot * 2, pk._key.L2)
    hist2.iupdate(dv, positions, 2, pk)
    monkeypatch.delenv("FPHE_FOLD_RAISE")
    assert hist2.to_signed_ints(pk.ns) == ([c.c for c in want], [c.exp for c in want])
    # cumsum with step 1 over two chunks
    cv = P.CiphertextVector.from_signed_ints([c.c for c in src[:40]], [c.exp for c in src[:40]], pk.ns, pk._key.L2)
    cv.chunking_cumsum_with_step(pk, [25, 15], 1)
    ref = list(src[:40])
    O.chunking_cumsum_with_step(opk, ref, [25, 15], 1)
    assert cv.to_signed_ints(pk.ns) == ([c.c for c in ref], [c.exp for c in ref])
    # the reference's pickle state at L2 = 256, and back
    state = wire.ciphertext_vector_to_bincode(dv, pk)
    back, used = wire.ciphertext_vector_from_bincode(state, pk)
    assert used == len(state) and back.to_signed_ints(pk.ns) == dv.to_signed_ints(pk.ns)
    raw = pickle.loads(pickle.dumps(dv))
    assert raw.to_signed_ints() == ([c.c for c in src], [c.exp for c in src])


@pytest.mark.parametrize("bits", [1024, 2048])
def test_decrypt_latency_kernel_matches_throughput(bits):
    """Decryptions of at most 4,096 elements run their half-size modexps on the one-element-
    per-wave kernel (wide_dev.h k_pow_half_wide); 4,097 take the throughput kernel
    (k_pow_half27).  The same ciphertexts -- device-RNG encryptions of both signs, the edge
    values, and sums whose exponents were aligned -- decrypt to the same plaintexts either way,
    and the short ones round-trip to the encoded inputs."""
    import json as _json
    with open(os.path.join(HERE, "golden", f"paillier_{bits}.json")) as f:
        fx = _json.load(f)
    sk, pk, coder = P.keypair_from_primes(int(fx["p"], 16), int(fx["q"], 16))
    g = torch.Generator().manual_seed(bits)
    x = torch.randn(4097, generator=g, dtype=torch.float64) * 4
    x[:6] = torch.tensor([0.0, 1e-300, -1e-300, 1e300, -1e300, -1.0], dtype=torch.float64)
    xd = x.cuda()
    v = pk.encrypt_encoded(coder.encode_f64_vec(xd), True)
    v = v.add(pk, pk.encrypt_encoded(coder.encode_f64_vec(xd.flip(0) * 1e-3), True))
    big = sk.decrypt_to_encoded(v).to_ints()
    for n in (4096, 37, 1):
        small = sk.decrypt_to_encoded(v.slice(0, n)).to_ints()
        assert small == (big[0][:n], big[1][:n]), n


@pytest.mark.parametrize("bits", [1024, 2048])
def test_encrypt_latency_kernel_matches_throughput(bits):
    """Obfuscated public-key encryptions of at most 2,048 elements run on the one-element-per-
    wave kernel (wide_dev.h k_encrypt_wide, M-form written directly); 2,049 take k_encrypt27 +
    k_mont_const27.  With the same injected r the integers agree, for float significands of
    both signs (negative ciphertexts), zero, and encoded negative integers (m > n/4); the short
    ones also decrypt to their significands."""
    import json as _json
    import random as _random
    with open(os.path.join(HERE, "golden", f"paillier_{bits}.json")) as f:
        fx = _json.load(f)
    sk, pk, coder = P.keypair_from_primes(int(fx["p"], 16), int(fx["q"], 16), keyholder=False)
    rng = _random.Random(bits)
    n = 2049
    x = torch.tensor([rng.uniform(-5, 5) for _ in range(n)], dtype=torch.float64)
    x[:3] = torch.tensor([0.0, -1e-300, 1e300], dtype=torch.float64)
    pv = coder.encode_f64_vec(x.cuda())
    iv = coder.encode_i64_vec(torch.tensor([-7, 5, -(1 << 40)] * 683, dtype=torch.int64).cuda())
    rs = [1 + rng.randrange(pk.n - 1) for _ in range(n)]
    for v in (pv, iv):
        big = pk.encrypt_encoded(v, True, r=rs).to_signed_ints(pk.ns)
        for m in (2048, 5, 1):
            sub = v._gather(torch.arange(m))
            small = pk.encrypt_encoded(sub, True, r=rs[:m])
            assert small.to_signed_ints(pk.ns) == (big[0][:m], big[1][:m]), m
        assert sk.decrypt_to_encoded(small).to_ints()[0] == [s_ % pk.n for s_ in v._gather(torch.arange(1)).to_ints()[0]]


@pytest.mark.parametrize("bits", [1024, 2048])
def test_keyholder_encrypt_latency_kernel_matches_throughput(monkeypatch, bits):
    """Key-holder encryptions with device-drawn (z_p, z_q) of at most 4,096 elements raise
    z_s^s mod s^2 on the one-element-per-wave kernel (wide_dev.h k_pow_half_enc_wide); 4,097
    take k_pow_half27<., ., true, true>.  With the nonce fixed, element i draws the same
    (z_p, z_q) in both calls (its index's stream), so the ciphertexts agree; they decrypt to
    the significands."""
    import json as _json
    with open(os.path.join(HERE, "golden", f"paillier_{bits}.json")) as f:
        fx = _json.load(f)
    sk, pk, coder = P.keypair_from_primes(int(fx["p"], 16), int(fx["q"], 16))
    assert pk.keyholder
    monkeypatch.setattr(pk._priv, "next_nonce", lambda: 777)
    n = 4097
    x = (torch.randn(n, generator=torch.Generator().manual_seed(bits), dtype=torch.float64) * 3).cuda()
    x[:2] = torch.tensor([0.0, -2.5], dtype=torch.float64)
    pv = coder.encode_f64_vec(x)
    big = pk.encrypt_encoded(pv, True).to_signed_ints(pk.ns)
    for m in (4096, 37, 1):
        small = pk.encrypt_encoded(pv._gather(torch.arange(m)), True)
        assert small.to_signed_ints(pk.ns) == (big[0][:m], big[1][:m]), m
    got = coder.decode_f64_vec(sk.decrypt_to_encoded(small)).cpu()
    assert got.tolist() == x[:1].cpu().tolist()
