// KeyArgs: the uniform key material every kernel takes by value (it lands in the kernarg segment
// -> SGPRs).  The pointers lead into the context's key blob (key_blob.h builds it and fills this
// struct).  Plain C++: the kernels, fate_phe.hip and the host-only blob builder share it.  It
// sits in the unnamed namespace, as everything internal to the library does, and the kernels'
// symbol names carry it.  Field order and types are the kernels' kernarg layout.
#pragma once
#include <stdint.h>

namespace fphe {
typedef uint32_t u32;  // as mont_dev.h
}  // namespace fphe

namespace {
using fphe::u32;

struct KeyArgs {
  const u32* N2;       // n^2                     [L2]
  const u32* N2_R2;    // R^2 mod n^2, R=2^(32 L2) [L2]
  const u32* N2_R1;    // R mod n^2 (Montgomery 1) [L2]
  const u32* n;        // n, padded               [L1+1]
  const u32* nm1;      // n-1                     [L1]
  const u32* max_int;  // floor(n/2)              [L1]
  const u32* n_mm;     // n - max_int             [L1]
  u32 n2_n0inv;
  int nbits;
  // private half (valid iff has_sk)
  const u32* P2; const u32* P2_R3; const u32* pm1; const u32* p; const u32* pinv2; const u32* hpR;
  const u32* Q2; const u32* Q2_R3; const u32* qm1; const u32* q; const u32* qinv2; const u32* hqR;
  const u32* pinvqR;   // p^{-1} mod q, times R_q mod q
  u32 p2_n0inv, p_n0inv, q2_n0inv, q_n0inv;
  int pm1_bits, qm1_bits;
  // reduced-radix engine (kernels27.h): LB-bit limbs (27 for n^2 of 2048-bit keys, 28 for
  // every other modulus), R = 2^(LB NL); the _27 suffix names the engine, not the radix
  const u32* N2_27; const u32* N2R1_27; const u32* N2R2_27;  // n^2, R mod n^2, R^2 mod n^2 [NL2]
  const u32* P2_27; const u32* P2R1_27; const u32* P2R2_27;  // p^2 ...                      [NLh]
  const u32* Q2_27; const u32* Q2R1_27; const u32* Q2R2_27;
  u32 n2_np27, p2_np27, q2_np27;                             // -N^{-1} mod 2^LB
  const u32* Nn_27; const u32* NnR1_27; const u32* NnR2_27;  // n, R mod n, R^2 mod n    [NLh]
  u32 nn_np27, nn_inv27;                                     // -n^{-1}, n^{-1} mod 2^LB
  // key-holder (CRT) encryption, valid iff has_sk: r^n mod s^2 = r^(n mod s(s-1)) mod s^2,
  // recombined as x_p Kp + x_q Kq mod n^2 (Kp = q^2 (q^-2 mod p^2), Kq = p^2 (p^-2 mod q^2))
  const u32* ep; const u32* eq;          // n mod p(p-1), n mod q(q-1)           [L1]
  int ep_bits, eq_bits;
  const u32* KpR_27; const u32* KqR_27;  // Kp R, Kq R mod n^2 (R = 2^(LB NL2))         [NL2]
  // Montgomery-resident ciphertexts: vectors hold M(c) = c R mod n^2 with the
  // n^2 engine's R.  R^3 mod n^2 takes a plain value x to x R^2 in one product (inverses,
  // the key-holder nude factor); R_s^2 R^-1 mod s^2 takes M(c) mod s^2 to c R_s (decrypt).
  const u32* N2R3_27;                    // R^3 mod n^2                                  [NL2]
  const u32* P2RX_27; const u32* Q2RX_27;  // R_s^2 R^-1 mod s^2, s = p, q                [NLh]
  const u32* N2M1;                       // M(1) = R mod n^2 in 32-bit words (literal 1)  [L2]
  // key-holder encryption in two steps (FPHE_KH_SPLIT): z_s = r^(e_s)
  // mod s with e_p = q mod (p-1), e_q = p mod (q-1), on the engine of s (TPIs = L2/128 lanes,
  // at least 1), then x_s = z_s^s mod s^2 on the s^2 engine
  const u32* Ps_27; const u32* PsR2_27; const u32* PsR3_27;  // p, R_s^2, R_s^3 mod p      [NLs]
  const u32* Qs_27; const u32* QsR2_27; const u32* QsR3_27;
  u32 ps_np27, qs_np27;
  const u32* e1p; const u32* e1q;        // q mod (p-1), p mod (q-1)                   [LQ]
  int e1p_bits, e1q_bits, p_bits, q_bits;
};
}  // namespace
