// Okamoto-Uchiyama kernels on the reduced-radix engine (rust/fate_utils/crates/ou/src/lib.rs:
// 69-138).  Compiled once per radix like kernels_engine.inc: fate_phe.hip includes this file in
// the namespaces ou27 / ou28 (`using namespace fphe::r27 / r28`, powm27 of the same radix), so
// there is no include guard.
//
// An OU context keeps its ciphertext modulus n = p^2 q in the N2* slots of KeyArgs, so a
// ciphertext of L words runs the engine instantiation a Paillier n^2 of L words runs (TPI =
// L / 32 lanes per element).  Vectors hold M(c) = c R mod n, R = 2^(LB NL).
//
// encrypt: c = g^m h^r mod n with both bases fixed per key.  The context holds one table per
// base (fate_phe.hip ou_build_table), rows of NL limbs in Montgomery form:
//   row 0                                  M(1)
//   row 1 + (2^W - 1) i + (d - 1)          M(h^(d 2^(W i))),  i < hwin, d = 1 .. 2^W - 1
//   row 1 + (2^W - 1) (hwin + i) + (d - 1) M(g^(d 2^(W i))),  i < gwin
// An element multiplies the rows its window digits select: no squarings.  A digit that is 0 on
// every element of the wave costs nothing; where only some elements have a 0 they multiply by
// row 0.  Rows are fetched with per-lane global loads (lane q of an element reads limbs
// [LL q, LL q + LL) of its element's row): no buffer descriptor is ever chosen per lane.

template <int W>
constexpr u32 kOuDigits = (1u << W) - 1u;

// this lane's LL limbs of a table row -> registers / the LDS operand slot
__device__ __forceinline__ void ou_row_load(L27& A, const u32* __restrict__ row) {
#pragma unroll
  for (int j = 0; j < LL; j += 2) A.set2(j >> 1, row[j], j + 1 < LL ? row[j + 1] : 0u);
}
template <int TPI>
__device__ __forceinline__ void ou_row_to_slot(u32* bcol, u32 qoff, const u32* __restrict__ row) {
  u32 w[LL];
#pragma unroll
  for (int j = 0; j < LL; ++j) w[j] = row[j];
#if FPHE_TAB_BATCH
  __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
  for (int j = 0; j < LL; ++j) bcol[qoff + j * Geo<TPI>::E] = w[j];
}

// The windows of one exponent vector X [T][rows][64] (32-bit words, nwin windows of W bits):
// A <- A * prod_i row(base + i, digit_i).  `have` (wave-uniform) says whether A holds a value
// yet; the first product is a plain row load.  `live` is false on the padding lanes of the last
// wave tile, whose exponent words are not read as digits.
template <int TPI, int W>
__device__ __forceinline__ void ou_fixed_base(L27& A, bool& have, const __amdgpu_buffer_rsrc_t& Xr, u32 col, u32 nwin,
                                              bool live, const u32* __restrict__ tab, u32 win0, u32* bcol, u32 qoff,
                                              const Mod<TPI>& N, u32 np, int q) {
  static_assert(32 % W == 0, "windows do not straddle words");
  constexpr u32 PER = 32 / W, NL = Geo<TPI>::NL;
  const u32 nwords = (nwin + PER - 1) / PER;
#pragma unroll 1
  for (u32 k = 0; k < nwords; ++k) {
    u32 wv = __builtin_amdgcn_raw_buffer_load_b32(Xr, (col + 64u * k) * 4u, 0, 0);
    wv = live ? wv : 0u;
    if (!__builtin_amdgcn_readfirstlane((u32)(__ballot(wv != 0u) != 0ull))) continue;  // wave-uniform
#pragma unroll 1
    for (u32 t = 0; t < PER; ++t) {
      const u32 wi = k * PER + t;
      if (wi >= nwin) break;  // wave-uniform: a partial top word never indexes past the table
      const u32 d = (wv >> (W * t)) & kOuDigits<W>;
      if (!__builtin_amdgcn_readfirstlane((u32)(__ballot(d != 0u) != 0ull))) continue;
      const u32 r = d ? 1u + kOuDigits<W> * (win0 + wi) + (d - 1u) : 0u;
      const u32* row = tab + (size_t)r * NL + (u32)q * LL;
      if (!have) {
        ou_row_load(A, row);
        have = true;
      } else {
        ou_row_to_slot<TPI>(bcol, qoff, row);
        mont_mul<TPI>(A, bcol, N, np, q);
      }
    }
  }
}

// ======================================================================================
// encrypt (ou/src/lib.rs:100-108): C = M(g^m h^r mod n).  r [T][L][64] in [1, n-1] (drawn by
// k_draw_r<L> or injected), m [T][lp][64] with lp <= L/2.  The reference leaves the product of
// its two powm results unreduced; this writes the canonical residue.
// ======================================================================================
template <int L, int W>
__global__ __launch_bounds__(kBlock) FPHE_OCC_MISC void k_ou_encrypt27(KeyArgs K, const u32* __restrict__ tab, u32 hwin,
                                                         const u32* __restrict__ P, u32 lp,
                                                         const u32* __restrict__ rin, size_t count,
                                                         u32* __restrict__ Cout, u32 ldsw) {
  constexpr int TPI = L / 32;
  using G = Geo<TPI>;
  constexpr int E = G::E;
  constexpr u32 L32 = L;
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  G g;
  const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 gw = blockIdx.x * kWavesPerBlock + wib, nw = gridDim.x * kWavesPerBlock;
  u32* bcol = lds + wib * ldsw * E + g.e;
  const u32 qoff = lds_qoff<TPI>(g.q);
  Mod<TPI> N;
  N.init(K.N2_27, g.q);
  const u32 np = K.n2_np27;
  const u32 nwt = (u32)((count + E - 1) / E);
  for (u32 wt = gw; wt < nwt; wt += nw) {
    const size_t ebase = (size_t)wt * E;
    const u32 tile = (u32)(ebase >> 6);
    const u32 col = (u32)(ebase & 63) + (u32)g.e;
    const bool live = ebase + g.e < count;
    const __amdgpu_buffer_rsrc_t Rr = rsrc(rin + (size_t)tile * L32 * FPHE_WAVE, L32 * 256u);
    const __amdgpu_buffer_rsrc_t Pr = rsrc(P + (size_t)tile * lp * FPHE_WAVE, lp * 256u);
    L27 A;
    bool have = false;
    ou_fixed_base<TPI, W>(A, have, Rr, col, hwin, live, tab, 0u, bcol, qoff, N, np, g.q);
    ou_fixed_base<TPI, W>(A, have, Pr, col, lp * (32u / W), live, tab, hwin, bcol, qoff, N, np, g.q);
    if (!have) ou_row_load(A, tab + (u32)g.q * LL);  // r = m = 0 on every lane: M(1)
    finalize<TPI>(A, N, g.q);
    const ColIO Co = colio(Cout + (size_t)tile * L32 * FPHE_WAVE, L32, col, 32u * g.q);
    store_chunk<TPI>(A, g.q, [&](int k, u32 v) { Co.st(k, v); });
  }
}

// ======================================================================================
// decrypt, modexp phase (ou/src/lib.rs:120-131): y = c^(p-1) mod p^2 into Y [T][L][64]; the
// L-function and the h_p product run in k_ou_decrypt_tail (fate_phe.hip, crt_tail).  p^2 has
// about 2/3 of n's bits: it runs on n's engine, zero-padded to its NL limbs (same R).  p^2
// divides n, so the stored M(c) = c R mod n is c R mod p^2 up to a multiple of p^2: one
// product by R mod p^2 reduces it (M(c) < R against a constant < N: < 2N, mont27_dev.h).
// ======================================================================================
template <int L, int W>
__global__ __launch_bounds__(kBlock) FPHE_OCC_POW void k_ou_decrypt27(KeyArgs K, const u32* __restrict__ C, size_t count,
                                                         u32* __restrict__ Y, u32* __restrict__ scratch, u32 ldsw) {
  constexpr int TPI = L / 32;
  using G = Geo<TPI>;
  constexpr int E = G::E;
  constexpr u32 L32 = L;
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  G g;
  const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 gw = blockIdx.x * kWavesPerBlock + wib, nw = gridDim.x * kWavesPerBlock;
  u32* bcol = lds + wib * ldsw * E + g.e;
  const u32 qoff = lds_qoff<TPI>(g.q);
  const Tile tb = make_tile(scratch + (size_t)gw * ((size_t)kTabEntries<W> * LL * FPHE_WAVE),
                            kTabEntries<W> * LL * 256u, g.lane);
  Mod<TPI> N;
  N.init(K.P2_27, g.q);
  const u32 np = K.p2_np27;
  const u32 nwt = (u32)((count + E - 1) / E);
  for (u32 wt = gw; wt < nwt; wt += nw) {
    const size_t ebase = (size_t)wt * E;
    const u32 tile = (u32)(ebase >> 6);
    const u32 col = (u32)(ebase & 63) + (u32)g.e;
    const ColIO Ci = colio(C + (size_t)tile * L32 * FPHE_WAVE, L32, col, 32u * g.q);
    const ColIO Yo = colio(Y + (size_t)tile * L32 * FPHE_WAVE, L32, col, 32u * g.q);
    L27 A;
    load_chunk<TPI>(A, CSH * g.q, [&](int k) { return Ci.ld(k); });
    const_to_slot<TPI>(bcol, qoff, K.P2R1_27, g.q);
    mont_mul<TPI>(A, bcol, N, np, g.q);  // c R mod p^2, < 2N
    powm27<TPI, W>(A, bcol, qoff, tb, N, np, K.pm1, K.pm1_bits, g.q);
    one_to_slot<TPI>(bcol, qoff, g.q);
    mont_mul<TPI>(A, bcol, N, np, g.q);  // leave Montgomery form
    finalize<TPI>(A, N, g.q);
    store_chunk<TPI>(A, g.q, [&](int k, u32 v) { Yo.st(k, v); });
  }
}

// ======================================================================================
// inverse mod n (fixedpoint_ou neg / sub: invert mod n): Co = M(v^-1) for C = M(v).  Paillier's
// two steps (k_inv_n27 mod n, then the lift to n^2) do not apply to n = p^2 q: one safegcd on
// the full-width engine.  x = C^-1 = v^-1 R^-1, and mont(x, R^3) = v^-1 R.  need as k_inv_n27.
// ======================================================================================
template <int L>
__global__ __launch_bounds__(kBlock) void k_ou_inv27(KeyArgs K, const u32* __restrict__ C, size_t count,
                                                     const u8* __restrict__ need, u32* __restrict__ Co,
                                                     int32_t* __restrict__ err, u32 ldsw) {
  constexpr int TPI = L / 32;
  using G = Geo<TPI>;
  constexpr int E = G::E;
  constexpr u32 L32 = L;
  constexpr int kBatches = (49 * (L * 32) + 80) / 17 / LB + 2;  // Bernstein-Yang bound / LB, + margin
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  G g;
  const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 gw = blockIdx.x * kWavesPerBlock + wib, nw = gridDim.x * kWavesPerBlock;
  u32* bcol = lds + wib * ldsw * E + g.e;
  const u32 qoff = lds_qoff<TPI>(g.q);
  Mod<TPI> N;
  N.init(K.N2_27, g.q);
  const u32 np = K.n2_np27;
  const u32 nwt = (u32)((count + E - 1) / E);
  for (u32 wt = gw; wt < nwt; wt += nw) {
    const size_t ebase = (size_t)wt * E;
    const u32 tile = (u32)(ebase >> 6);
    const u32 col = (u32)(ebase & 63) + (u32)g.e;
    const size_t elem = ebase + g.e;
    const bool nd = elem < count && (need == nullptr || need[elem] != 0);
    if (!__any(nd)) continue;
    const ColIO Ci = colio(C + (size_t)tile * L32 * FPHE_WAVE, L32, col, 32u * g.q);
    L27 A;
    load_chunk<TPI>(A, CSH * g.q, [&](int k) { return Ci.ld(k); });
    const bool ok = inv_mod<TPI>(A, N, K.nn_inv27, kBatches, g.q);
    const_to_slot<TPI>(bcol, qoff, K.N2R3_27, g.q);
    mont_mul<TPI>(A, bcol, N, np, g.q);
    finalize<TPI>(A, N, g.q);
    const ColIO Oo = colio(Co + (size_t)tile * L32 * FPHE_WAVE, L32, col, 32u * g.q);
    store_chunk<TPI>(A, g.q, [&](int k, u32 v) {
      if (nd) Oo.st(k, v);
    });
    if (g.q == 0 && nd && !ok) set_err(err, FPHE_EF_NOT_INVERTIBLE);
  }
}

struct Kern {
  template <int L, int W> static auto encrypt() { return k_ou_encrypt27<L, W>; }
  template <int L, int W> static auto decrypt() { return k_ou_decrypt27<L, W>; }
  template <int L> static auto inv() { return k_ou_inv27<L>; }
};
