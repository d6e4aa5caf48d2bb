// Whole-vector utility kernels: element permutation (fphe_permute), the reference's signed
// integers (fphe_export_signed / fphe_import_signed) and the shader-clock stamps.
#pragma once
#include "mont_dev.h"

namespace {
using namespace fphe;

// ---- element permutation of tile-major vectors (gather / scatter) ---------------------
// One thread per 32-bit word of the contiguous side, so that side is read or written fully
// coalesced; the indexed side follows idx (stable sorts and slices keep it mostly local).
// Indexes outside [0, nspace) are skipped; the host checks them before the call.
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_permute(const u32* __restrict__ Cin, const u8* __restrict__ sin,
                                                 const int32_t* __restrict__ ein, u32 L,
                                                 const int64_t* __restrict__ idx, size_t count, size_t nspace,
                                                 u32* __restrict__ Cout, u8* __restrict__ sout,
                                                 int32_t* __restrict__ eout) {
  const size_t per_tile = (size_t)L * FPHE_WAVE;
  const size_t total = ((count + FPHE_WAVE - 1) / FPHE_WAVE) * per_tile;
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
    const size_t tile = o / per_tile, rem = o - tile * per_tile;
    const u32 w = (u32)(rem >> 6), col = (u32)(rem & 63);
    const size_t i = tile * FPHE_WAVE + col;  // position on the contiguous side
    if (i >= count) continue;
    const int64_t j = idx[i];
    if (j < 0 || (size_t)j >= nspace) continue;
    const size_t oj = ((size_t)j >> 6) * per_tile + (size_t)w * FPHE_WAVE + ((size_t)j & 63);
    if (SCATTER) {
      if (Cin) Cout[oj] = Cin[o];
      if (w == 0) {
        if (sin) sout[j] = sin[i];
        if (ein) eout[j] = ein[i];
      }
    } else {
      if (Cin) Cout[o] = Cin[oj];
      if (w == 0) {
        if (sin) sout[i] = sin[j];
        if (ein) eout[i] = ein[j];
      }
    }
  }
}

// ---- (C, sign) <-> the reference's signed integers ------------------------------------
// The reference's ciphertext is the signed rug::Integer C - sign n^2 (canonical C, SURVEY.md
// §0 fact 1).  Export writes its magnitude as element-major LSF words and a negative flag;
// import is the inverse.  One thread per element; the tile-major side is coalesced.
__global__ __launch_bounds__(256) void k_export_signed(const u32* __restrict__ N2, u32 L, const u32* __restrict__ C,
                                                       const u8* __restrict__ sign, size_t count,
                                                       u32* __restrict__ mag, u8* __restrict__ neg) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const u32* c = C + (e >> 6) * (size_t)L * FPHE_WAVE + (e & 63);
  u32* m = mag + e * L;
  u32 nz = 0;
  for (u32 w = 0; w < L; ++w) nz |= c[(size_t)w * FPHE_WAVE];
  const bool ng = sign[e] != 0 && nz != 0;
  u32 borrow = 0;
  for (u32 w = 0; w < L; ++w) {
    const u32 cw = c[(size_t)w * FPHE_WAVE];
    if (ng) {  // n^2 - C
      const u64 d = (u64)N2[w] - cw - borrow;
      m[w] = (u32)d;
      borrow = (u32)(d >> 63);
    } else {
      m[w] = cw;
    }
  }
  neg[e] = ng ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_import_signed(const u32* __restrict__ N2, u32 L, const u32* __restrict__ mag,
                                                       const u8* __restrict__ neg, size_t count, u32* __restrict__ C,
                                                       u8* __restrict__ sign) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  u32* c = C + (e >> 6) * (size_t)L * FPHE_WAVE + (e & 63);
  const u32* m = mag + e * L;
  u32 nz = 0;
  for (u32 w = 0; w < L; ++w) nz |= m[w];
  const bool ng = neg[e] != 0 && nz != 0;
  u32 borrow = 0;
  for (u32 w = 0; w < L; ++w) {
    if (ng) {  // canonical n^2 - |c|
      const u64 d = (u64)N2[w] - m[w] - borrow;
      c[(size_t)w * FPHE_WAVE] = (u32)d;
      borrow = (u32)(d >> 63);
    } else {
      c[(size_t)w * FPHE_WAVE] = m[w];
    }
  }
  sign[e] = ng ? 1 : 0;
}
}  // namespace

extern "C" {
// Shader-clock stamps (diagnostics; bench.py's per-leg clock).  `blocks`
// one-wave workgroups; lane 0 of block b writes {its CU's place -- XCC id << 16 | the SE, SH
// and CU fields of HW_ID --, the shader-clock counter (clock64: s_memtime, counts SCLK
// cycles), the constant-rate counter (wall_clock64)} to out[3b .. 3b+2] with vector stores.
// The shader-clock counters of different CUs are not synchronised (a before/after pair from
// two CUs of one XCD can even run backwards), so the host pairs two stamps queued around a
// launch by CU; with a few thousand blocks every CU is stamped on both sides.
__global__ __launch_bounds__(64) void k_clock_stamp(unsigned long long* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const unsigned long long c = clock64();
  const unsigned long long w = wall_clock64();
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15u;   // HW_REG_XCC_ID
  const unsigned hw = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4) & 255u;    // HW_ID[15:8]
  out[3 * blockIdx.x] = (xcc << 16) | hw;
  out[3 * blockIdx.x + 1] = c;
  out[3 * blockIdx.x + 2] = w;
}
}  // extern "C"
