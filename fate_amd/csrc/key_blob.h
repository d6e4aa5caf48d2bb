// The key blob: every per-key constant the kernels read, derived on the host at context creation
// and uploaded once; KeyArgs (key_args.h) points into it.  Plain C++17, no HIP: fate_phe.hip
// calls build_paillier_blob / build_ou_blob, and a stand-alone program can (tests/test_key_blob.py
// pins the blobs of the committed keys).  Internal to the library, hence the unnamed namespace.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

#include "../../include/fate_phe.h"
#include "host_bn.h"
#include "key_args.h"
#include "radix.h"

namespace {

using hbn::Limbs;

constexpr int kOuWin = 4;  // fixed-base window of k_ou_encrypt27 (table size against L2)

inline Limbs from_words(const uint32_t* w, size_t n) { return hbn::norm(Limbs(w, w + n)); }

// little-endian 32-bit words -> nl limbs of lb bits (the engine radix of the modulus)
inline Limbs to_radix(const Limbs& v, int nl, int lb) {
  Limbs o((size_t)nl, 0u);
  for (int i = 0; i < nl; ++i) {
    const size_t bit = (size_t)lb * i, w = bit >> 5;
    const unsigned off = (unsigned)(bit & 31);
    uint64_t x = w < v.size() ? v[w] : 0u;
    if (w + 1 < v.size()) x |= (uint64_t)v[w + 1] << 32;
    o[(size_t)i] = (u32)(x >> off) & ((1u << lb) - 1u);
  }
  return o;
}

// A blob under construction, with the KeyArgs and the context scalars that go with it.  Each
// put() names the KeyArgs pointer it fills; the pointers themselves exist once the blob has a
// device address (resolve).
struct KeyBlob {
  using Field = const u32* KeyArgs::*;
  std::vector<u32> words;
  std::vector<std::pair<Field, size_t>> fixups;  // (field, word offset of its section)
  KeyArgs K{};                                   // the scalar fields; pointers are null until resolve()
  // the context's scalars (fphe_ctx)
  int L1 = 0, L2 = 0, LQ = 0;
  bool has_sk = false, kh_direct = false;
  u32 ou_hwin = 0;    // OU: windows of h's part of the fixed-base table,
  size_t ou_tab = 0;  // and the table's word offset

  // v zero-padded to len words (throws if it does not fit), as a 16-byte aligned section
  void put(Field f, const Limbs& v, size_t len) {
    fixups.emplace_back(f, words.size());
    const Limbs p = hbn::padded(v, len);
    words.insert(words.end(), p.begin(), p.end());
    while (words.size() % 4) words.push_back(0);
  }

  // The engine-radix constants of an odd modulus N on the engine of `tpi` lanes per element
  // (NL = rad_ll(tpi) tpi limbs of LB = rad_lb(tpi) bits, R = 2^(LB NL)): N, then R^k mod N for
  // each k = 1, 2, 3 whose field is given, and -N^-1 mod 2^LB.
  struct Engine {
    Field N, R1, R2, R3;
    u32 KeyArgs::*np;
  };
  void put_modulus(const Engine& f, const Limbs& N, int tpi) {
    const int lb = fphe::rad_lb(tpi), nl = fphe::rad_ll(tpi) * tpi;
    put(f.N, to_radix(N, nl, lb), nl);
    const Field rk[3] = {f.R1, f.R2, f.R3};
    for (int k = 1; k <= 3; ++k)
      if (rk[k - 1]) put(rk[k - 1], to_radix(hbn::pow2_mod((size_t)k * lb * nl, N), nl, lb), nl);
    K.*f.np = hbn::neg_inv32(N[0]) & ((1u << lb) - 1u);
  }

  // KeyArgs for the blob at `base`
  KeyArgs resolve(const u32* base) const {
    KeyArgs r = K;
    for (const auto& fx : fixups) r.*fx.first = base + fx.second;
    return r;
  }
};

// Host Montgomery products (32-bit CIOS, R = 2^(32 L)) for the setup work hbn::mod is too slow
// for: g^(p-1) mod p^2 and the ~10^4 products of the fixed-base tables.
struct HostMont {
  Limbs N, R2;
  size_t L;
  u32 n0;
  HostMont(const Limbs& n, size_t l) : N(hbn::padded(n, l)), R2(hbn::padded(hbn::pow2_mod(64 * l, n), l)), L(l),
                                       n0(hbn::neg_inv32(n[0])) {}
  // a b R^-1 mod N for a, b < N (L words each)
  Limbs mul(const Limbs& a, const Limbs& b) const {
    std::vector<u32> t(L + 2, 0u);
    for (size_t i = 0; i < L; ++i) {
      uint64_t c = 0;
      for (size_t j = 0; j < L; ++j) {
        const uint64_t s = (uint64_t)a[j] * b[i] + t[j] + c;
        t[j] = (u32)s;
        c = s >> 32;
      }
      uint64_t s = (uint64_t)t[L] + c;
      t[L] = (u32)s;
      t[L + 1] = (u32)(s >> 32);
      const u32 m = t[0] * n0;
      c = ((uint64_t)m * N[0] + t[0]) >> 32;
      for (size_t j = 1; j < L; ++j) {
        s = (uint64_t)m * N[j] + t[j] + c;
        t[j - 1] = (u32)s;
        c = s >> 32;
      }
      s = (uint64_t)t[L] + c;
      t[L - 1] = (u32)s;
      t[L] = t[L + 1] + (u32)(s >> 32);
    }
    // t < 2N: one conditional subtraction, in place
    bool ge = t[L] != 0;
    if (!ge) {
      ge = true;  // t == N counts
      for (size_t j = L; j-- > 0;)
        if (t[j] != N[j]) { ge = t[j] > N[j]; break; }
    }
    if (ge) {
      uint64_t br = 0;
      for (size_t j = 0; j < L; ++j) {
        const uint64_t d = (uint64_t)t[j] - N[j] - br;
        t[j] = (u32)d;
        br = d >> 63;
      }
    }
    t.resize(L);
    return t;
  }
  Limbs to(const Limbs& x) const { return mul(hbn::padded(x, L), R2); }  // x R
  Limbs from(const Limbs& X) const {                                       // X R^-1
    Limbs one(L, 0u);
    one[0] = 1;
    return mul(X, one);
  }
  // x^e mod N (plain in, plain out), x < N
  Limbs pow(const Limbs& x, const Limbs& e) const {
    const Limbs X = to(x);
    Limbs A = to(Limbs{1});
    for (size_t i = hbn::bitlen(e); i-- > 0;) {
      A = mul(A, A);
      if (hbn::bit(e, i)) A = mul(A, X);
    }
    return hbn::norm(from(A));
  }
};

// rows of the fixed-base table (ou_dev.h) for one base: M(base^(d 2^(W i))) for i < nwin,
// d = 1 .. 2^W - 1, as NL limbs of LB bits, appended to `out`.  Reng = 2^(LB NL) mod n.
inline void ou_table_rows(const HostMont& M, const Limbs& base, u32 nwin, const Limbs& Reng, int NL, int LB,
                          std::vector<u32>& out) {
  constexpr u32 D = (1u << kOuWin) - 1u;
  Limbs b = M.to(base);  // base^(2^(W i)) in the host's Montgomery form
  for (u32 i = 0; i < nwin; ++i) {
    Limbs e = b;
    for (u32 d = 1; d <= D; ++d) {
      const Limbs row = to_radix(hbn::norm(M.mul(e, Reng)), NL, LB);  // (x R32)(R_eng) / R32 = x R_eng
      out.insert(out.end(), row.begin(), row.end());
      e = M.mul(e, b);
    }
    b = e;  // base^(2^W 2^(W i))
  }
}

// Paillier: n (L1 words), and p, q (LQ words each) or both null for a public-only context.
// key_bits is even and in [256, 4096] (the caller checks); FPHE_ERR_KEY for a key that is not one.
inline fphe_status build_paillier_blob(uint32_t key_bits, const uint32_t* n_w, const uint32_t* p_w,
                                       const uint32_t* q_w, KeyBlob& B) {
  using KA = KeyArgs;
  // any even size up to 4096 bits (paillier/src/lib.rs:72-87 accepts any even size): the
  // kernels run the 1024-, 2048- or 4096-bit geometry with n zero-padded to it (R >= 4N
  // holds, so the lazy Montgomery bounds are unchanged).  Above 2048 bits n^2 spans 8 lanes
  // per element (TPI 8, 296 limbs of 28 bits) and n, p^2, q^2 the TPI-4 geometry.
  const int L1 = key_bits <= 1024 ? 32 : (key_bits <= 2048 ? 64 : 128), L2 = 2 * L1, LQ = L1 / 2;
  B.L1 = L1; B.L2 = L2; B.LQ = LQ;
  B.has_sk = p_w != nullptr;
  try {
    const Limbs n = from_words(n_w, L1);
    if (n.empty() || !(n[0] & 1)) return FPHE_ERR_KEY;
    if (hbn::bitlen(n) != key_bits) return FPHE_ERR_KEY;  // paillier/src/lib.rs:82 keeps bits(n)==k
    const Limbs N2 = hbn::mul(n, n);
    B.put(&KA::N2, N2, L2);
    B.put(&KA::N2_R2, hbn::pow2_mod((size_t)64 * L2, N2), L2);
    B.put(&KA::N2_R1, hbn::pow2_mod((size_t)32 * L2, N2), L2);
    B.put(&KA::n, n, L1 + 1);
    B.put(&KA::nm1, hbn::sub(n, Limbs{1}), L1);
    Limbs max_int = n;  // floor(n/2)
    for (size_t i = 0; i < max_int.size(); ++i)
      max_int[i] = (max_int[i] >> 1) | (i + 1 < max_int.size() ? max_int[i + 1] << 31 : 0);
    max_int = hbn::norm(max_int);
    B.put(&KA::max_int, max_int, L1);
    B.put(&KA::n_mm, hbn::sub(n, max_int), L1);
    B.K.n2_n0inv = hbn::neg_inv32(N2[0]);
    B.K.nbits = (int)key_bits;
    // engine limbs: n^2 at TPI2 = L2/32 lanes, n / p^2 / q^2 at TPIh = L2/64, p / q at TPIs, each
    // in the radix of its engine (mont27_dev.h: 27 bits at TPI 4, 28 below); R = 2^(LB NL)
    const int TPI2 = L2 / 32, TPIh = L2 / 64, TPIs = L2 >= 128 ? L2 / 128 : 1;
    const int LB2 = fphe::rad_lb(TPI2), LBh = fphe::rad_lb(TPIh);
    const int NL2 = fphe::rad_ll(TPI2) * TPI2, NLh = fphe::rad_ll(TPIh) * TPIh;
    const Limbs R27 = hbn::pow2_mod((size_t)LB2 * NL2, N2);  // R of the n^2 engine
    B.put_modulus({&KA::N2_27, &KA::N2R1_27, &KA::N2R2_27, &KA::N2R3_27, &KA::n2_np27}, N2, TPI2);
    B.put(&KA::N2M1, R27, L2);
    B.put_modulus({&KA::Nn_27, &KA::NnR1_27, &KA::NnR2_27, nullptr, &KA::nn_np27}, n, TPIh);
    B.K.nn_inv27 = (0u - hbn::neg_inv32(n[0])) & ((1u << LBh) - 1u);
    if (!B.has_sk) return FPHE_OK;

    Limbs p = from_words(p_w, LQ), q = from_words(q_w, LQ);
    if (hbn::cmp(p, q) == 0) return FPHE_ERR_KEY;
    if (hbn::cmp(p, q) > 0) std::swap(p, q);  // SK::new keeps p < q (paillier/src/lib.rs:127)
    if (hbn::cmp(hbn::mul(p, q), n) != 0) return FPHE_ERR_KEY;
    if (!(p[0] & 1) || !(q[0] & 1)) return FPHE_ERR_KEY;
    const Limbs P2 = hbn::mul(p, p), Q2 = hbn::mul(q, q);
    const Limbs pm1 = hbn::sub(p, Limbs{1}), qm1 = hbn::sub(q, Limbs{1});
    // h_p = ((g^(p-1) mod p^2 - 1)/p)^{-1} mod p with g = n+1 (paillier/src/lib.rs:131-137);
    // (1+n)^(p-1) = 1 + (p-1) n (mod p^2), so the L-value is (p-1) q mod p.
    auto hval = [&](const Limbs& s, const Limbs& t) {
      Limbs Lv = hbn::mod(hbn::mul(hbn::sub(s, Limbs{1}), t), s);
      return hbn::inv_mod(Lv, s);
    };
    // x R_s mod s with the 32-bit R_s = 2^(32 LQ) of crt_tail / crt_combine
    auto mont32 = [&](const Limbs& x, const Limbs& s) {
      return hbn::mod(hbn::mul(x, hbn::pow2_mod((size_t)32 * LQ, s)), s);
    };
    B.put(&KA::P2, P2, L1);
    B.put(&KA::P2_R3, hbn::pow2_mod((size_t)96 * L1, P2), L1);
    B.put(&KA::pm1, pm1, LQ + 1);
    B.put(&KA::p, p, LQ);
    B.put(&KA::pinv2, hbn::inv_pow2(p, LQ), LQ);
    B.put(&KA::hpR, mont32(hval(p, q), p), LQ);
    B.put(&KA::Q2, Q2, L1);
    B.put(&KA::Q2_R3, hbn::pow2_mod((size_t)96 * L1, Q2), L1);
    B.put(&KA::qm1, qm1, LQ + 1);
    B.put(&KA::q, q, LQ);
    B.put(&KA::qinv2, hbn::inv_pow2(q, LQ), LQ);
    B.put(&KA::hqR, mont32(hval(q, p), q), LQ);
    B.put(&KA::pinvqR, mont32(hbn::inv_mod(p, q), q), LQ);
    B.put_modulus({&KA::P2_27, &KA::P2R1_27, &KA::P2R2_27, nullptr, &KA::p2_np27}, P2, TPIh);
    B.put_modulus({&KA::Q2_27, &KA::Q2R1_27, &KA::Q2R2_27, nullptr, &KA::q2_np27}, Q2, TPIh);
    // R_s^2 R^-1 mod s^2 (R of n^2, R_s of s^2): mont_s(M(c) mod s^2, .) = c R_s
    auto rx = [&](const Limbs& S2) {
      const Limbs Rn = hbn::pow2_mod((size_t)LB2 * NL2, S2);
      return hbn::mod(hbn::mul(hbn::pow2_mod((size_t)2 * LBh * NLh, S2), hbn::inv_mod(Rn, S2)), S2);
    };
    B.put(&KA::P2RX_27, to_radix(rx(P2), NLh, LBh), NLh);
    B.put(&KA::Q2RX_27, to_radix(rx(Q2), NLh, LBh), NLh);
    B.K.p2_n0inv = hbn::neg_inv32(P2[0]); B.K.p_n0inv = hbn::neg_inv32(p[0]);
    B.K.q2_n0inv = hbn::neg_inv32(Q2[0]); B.K.q_n0inv = hbn::neg_inv32(q[0]);
    B.K.pm1_bits = (int)hbn::bitlen(pm1); B.K.qm1_bits = (int)hbn::bitlen(qm1);
    // CRT encryption constants
    const Limbs ep = hbn::mod(n, hbn::mul(p, pm1)), eq = hbn::mod(n, hbn::mul(q, qm1));
    B.put(&KA::ep, ep, L1);
    B.put(&KA::eq, eq, L1);
    B.K.ep_bits = (int)hbn::bitlen(ep); B.K.eq_bits = (int)hbn::bitlen(eq);
    // the split key-holder modexp's constants (KeyArgs)
    B.put_modulus({&KA::Ps_27, nullptr, &KA::PsR2_27, &KA::PsR3_27, &KA::ps_np27}, p, TPIs);
    B.put_modulus({&KA::Qs_27, nullptr, &KA::QsR2_27, &KA::QsR3_27, &KA::qs_np27}, q, TPIs);
    const Limbs e1p = hbn::mod(q, pm1), e1q = hbn::mod(p, qm1);
    B.put(&KA::e1p, e1p, LQ);
    B.put(&KA::e1q, e1q, LQ);
    B.K.e1p_bits = (int)hbn::bitlen(e1p); B.K.e1q_bits = (int)hbn::bitlen(e1q);
    B.K.p_bits = (int)hbn::bitlen(p); B.K.q_bits = (int)hbn::bitlen(q);
    // the key holder may draw (z_p, z_q) directly when gcd(q, p - 1) = gcd(p, q - 1) = 1; p, q
    // prime: gcd(q, p - 1) = 1 iff q does not divide p - 1 (and likewise)
    B.kh_direct = !hbn::is_zero(hbn::mod(pm1, q)) && !hbn::is_zero(hbn::mod(qm1, p));
    const Limbs Kp = hbn::mul(Q2, hbn::inv_mod(hbn::mod(Q2, P2), P2));  // < n^2
    const Limbs Kq = hbn::mul(P2, hbn::inv_mod(hbn::mod(P2, Q2), Q2));
    B.put(&KA::KpR_27, to_radix(hbn::mod(hbn::mul(Kp, R27), N2), NL2, LB2), NL2);
    B.put(&KA::KqR_27, to_radix(hbn::mod(hbn::mul(Kq, R27), N2), NL2, LB2), NL2);
    return FPHE_OK;
  } catch (...) {
    return FPHE_ERR_KEY;
  }
}

// Okamoto-Uchiyama (ou/src/lib.rs:69-138): n = p^2 q, g, h (L2 words each), and p, q (L1 words
// each) or both null.  The N2* slots of KeyArgs hold n, so the modulus-only kernels serve an OU
// context as they are.  key_bits is even and in [1024, 4096] (the caller checks).
inline fphe_status build_ou_blob(uint32_t key_bits, const uint32_t* n_w, const uint32_t* g_w, const uint32_t* h_w,
                                 const uint32_t* p_w, const uint32_t* q_w, KeyBlob& B) {
  using KA = KeyArgs;
  const int L2 = key_bits <= 2048 ? 64 : 128, L1 = L2 / 2;
  B.L1 = L1; B.L2 = L2; B.LQ = L1 / 2;
  B.has_sk = p_w != nullptr;
  try {
    const Limbs n = from_words(n_w, L2), g = from_words(g_w, L2), h = from_words(h_w, L2);
    if (n.empty() || !(n[0] & 1)) return FPHE_ERR_KEY;
    if (hbn::bitlen(n) != key_bits) return FPHE_ERR_KEY;  // ou/src/lib.rs:80 keeps bits(n) == bit_length
    if (g.empty() || h.empty() || hbn::cmp(g, n) >= 0 || hbn::cmp(h, n) >= 0) return FPHE_ERR_KEY;
    const int TPI2 = L2 / 32, LB2 = fphe::rad_lb(TPI2), NL2 = fphe::rad_ll(TPI2) * TPI2;
    const Limbs Reng = hbn::pow2_mod((size_t)LB2 * NL2, n);
    B.put(&KA::N2, n, L2);
    B.put(&KA::n, n, L2 + 1);
    B.put(&KA::nm1, hbn::sub(n, Limbs{1}), L2);
    B.put_modulus({&KA::N2_27, &KA::N2R1_27, &KA::N2R2_27, &KA::N2R3_27, &KA::n2_np27}, n, TPI2);
    B.put(&KA::N2M1, Reng, L2);
    B.K.n2_n0inv = hbn::neg_inv32(n[0]);
    B.K.nbits = (int)key_bits;
    B.K.nn_inv27 = (0u - B.K.n2_n0inv) & ((1u << LB2) - 1u);  // n^-1 mod 2^LB, k_ou_inv27's safegcd
    if (B.has_sk) {
      const Limbs p = from_words(p_w, L1), q = from_words(q_w, L1);
      if (p.empty() || q.empty() || !(p[0] & 1) || !(q[0] & 1)) return FPHE_ERR_KEY;
      if (hbn::cmp(p, q) == 0) return FPHE_ERR_KEY;
      const Limbs P2 = hbn::mul(p, p);
      if (hbn::cmp(hbn::mul(P2, q), n) != 0) return FPHE_ERR_KEY;
      const Limbs pm1 = hbn::sub(p, Limbs{1});
      // h_p = L(g^(p-1) mod p^2)^-1 mod p, L(x) = (x - 1) / p (ou/src/lib.rs:120-131); a g whose
      // power is 1 has no inverse: inv_mod throws, FPHE_ERR_KEY
      const HostMont MP(P2, (size_t)L2);
      const Limbs y = MP.pow(hbn::mod(g, P2), pm1);
      if (y.empty()) return FPHE_ERR_KEY;
      const Limbs ym1 = hbn::sub(y, Limbs{1});
      // exact quotient (y - 1) / p by the inverse of p mod 2^(32 L1), as crt_tail does
      Limbs Lg = hbn::mul(hbn::padded(ym1, (size_t)L2), hbn::inv_pow2(p, (size_t)L1));
      Lg.resize((size_t)L1, 0u);
      const Limbs hp = hbn::inv_mod(hbn::norm(Lg), p);
      B.put_modulus({&KA::P2_27, &KA::P2R1_27, nullptr, nullptr, &KA::p2_np27}, P2, TPI2);
      B.put(&KA::pm1, pm1, L1 + 1);
      B.put(&KA::p, p, L1);
      B.put(&KA::pinv2, hbn::inv_pow2(p, (size_t)L1), L1);
      B.put(&KA::hpR, hbn::mod(hbn::mul(hp, hbn::pow2_mod((size_t)32 * L1, p)), p), L1);
      B.K.p_n0inv = hbn::neg_inv32(p[0]);
      B.K.pm1_bits = (int)hbn::bitlen(pm1);
      B.K.p_bits = (int)hbn::bitlen(p);
    }
    // fixed-base tables (ou_dev.h), 64-word aligned: row 0 = M(1), then h's windows over bits(n),
    // then g's over the L1 plaintext words a call may pass
    const u32 hwin = (key_bits + kOuWin - 1) / kOuWin, gwin = (u32)L1 * 32u / kOuWin;
    std::vector<u32>& blob = B.words;
    while (blob.size() % 64) blob.push_back(0);
    B.ou_tab = blob.size();
    B.ou_hwin = hwin;
    const HostMont MN(n, (size_t)L2);
    const Limbs RengP = hbn::padded(Reng, (size_t)L2);
    const Limbs one = to_radix(Reng, NL2, LB2);
    blob.reserve(blob.size() + (size_t)(1 + ((1u << kOuWin) - 1u) * (hwin + gwin)) * NL2);
    blob.insert(blob.end(), one.begin(), one.end());
    ou_table_rows(MN, h, hwin, RengP, NL2, LB2, blob);
    ou_table_rows(MN, g, gwin, RengP, NL2, LB2, blob);
    return FPHE_OK;
  } catch (...) {
    return FPHE_ERR_KEY;
  }
}

}  // namespace
