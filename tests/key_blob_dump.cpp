// Stand-alone driver of the host-only key-blob builder (fate_amd/csrc/key_blob.h), compiled with
// g++ and run by tests/test_key_blob.py.  Usage: key_blob_dump CASES OUTDIR.  CASES holds one key
// per line,
//   NAME paillier BITS N P Q      or      NAME ou BITS N G H P Q
// with hexadecimal integers and "-" for an absent P, Q.  For each line the program prints
// "case NAME status S" and, for status 0, the blob's length, every KeyArgs field (pointers as
// word offsets into the blob, -1 for null), the context scalars and "end"; the blob itself goes
// to OUTDIR/NAME.blob.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../fate_amd/csrc/key_blob.h"

#define KEYARGS_POINTERS(X)                                                                              \
  X(N2) X(N2_R2) X(N2_R1) X(n) X(nm1) X(max_int) X(n_mm) X(P2) X(P2_R3) X(pm1) X(p) X(pinv2) X(hpR)     \
  X(Q2) X(Q2_R3) X(qm1) X(q) X(qinv2) X(hqR) X(pinvqR) X(N2_27) X(N2R1_27) X(N2R2_27) X(P2_27)          \
  X(P2R1_27) X(P2R2_27) X(Q2_27) X(Q2R1_27) X(Q2R2_27) X(Nn_27) X(NnR1_27) X(NnR2_27) X(ep) X(eq)       \
  X(KpR_27) X(KqR_27) X(N2R3_27) X(P2RX_27) X(Q2RX_27) X(N2M1) X(Ps_27) X(PsR2_27) X(PsR3_27) X(Qs_27)  \
  X(QsR2_27) X(QsR3_27) X(e1p) X(e1q)
#define KEYARGS_SCALARS(X)                                                                               \
  X(n2_n0inv) X(nbits) X(p2_n0inv) X(p_n0inv) X(q2_n0inv) X(q_n0inv) X(pm1_bits) X(qm1_bits) X(n2_np27) \
  X(p2_np27) X(q2_np27) X(nn_np27) X(nn_inv27) X(ep_bits) X(eq_bits) X(ps_np27) X(qs_np27) X(e1p_bits)  \
  X(e1q_bits) X(p_bits) X(q_bits)

// hexadecimal -> 256 little-endian words (more than any argument's geometry), zero-padded
static std::vector<uint32_t> words_of(std::string hex) {
  if (hex.rfind("0x", 0) == 0) hex = hex.substr(2);
  std::vector<uint32_t> w(256, 0u);
  for (size_t i = 0; i < hex.size(); ++i) {
    const char ch = hex[hex.size() - 1 - i];
    const uint32_t v = ch <= '9' ? ch - '0' : (ch | 0x20) - 'a' + 10;
    if (i / 8 < w.size()) w[i / 8] |= v << (4 * (i % 8));
  }
  return w;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string name, scheme, tok;
    unsigned bits = 0;
    ss >> name >> scheme >> bits;
    std::vector<std::vector<uint32_t>> v;
    std::vector<const uint32_t*> a;
    while (ss >> tok) v.push_back(tok == "-" ? std::vector<uint32_t>() : words_of(tok));
    for (const auto& x : v) a.push_back(x.empty() ? nullptr : x.data());
    KeyBlob B;
    fphe_status st;
    if (scheme == "paillier" && a.size() == 3)
      st = build_paillier_blob(bits, a[0], a[1], a[2], B);
    else if (scheme == "ou" && a.size() == 5)
      st = build_ou_blob(bits, a[0], a[1], a[2], a[3], a[4], B);
    else
      return 2;
    printf("case %s status %d\n", name.c_str(), (int)st);
    if (st != FPHE_OK) continue;
    const uint32_t* base = B.words.data();
    const KeyArgs K = B.resolve(base);
    printf("blob_words %zu\nsizeof_KeyArgs %zu\n", B.words.size(), sizeof(KeyArgs));
#define X(f) printf("ptr %s %lld\n", #f, K.f ? (long long)(K.f - base) : -1LL);
    KEYARGS_POINTERS(X)
#undef X
#define X(f) printf("val %s %lld\n", #f, (long long)K.f);
    KEYARGS_SCALARS(X)
#undef X
    const bool ou = scheme == "ou";
    printf("ctx L1 %d\nctx L2 %d\nctx LQ %d\nctx has_sk %d\nctx kh_direct %d\nctx ou %d\nctx ou_hwin %u\nctx ou_tab %lld\n",
           B.L1, B.L2, B.LQ, (int)B.has_sk, (int)B.kh_direct, (int)ou, B.ou_hwin, ou ? (long long)B.ou_tab : -1LL);
    printf("end\n");
    FILE* f = fopen((std::string(argv[2]) + "/" + name + ".blob").c_str(), "wb");
    if (!f || fwrite(base, 4, B.words.size(), f) != B.words.size() || fclose(f) != 0) return 3;
  }
  return 0;
}
