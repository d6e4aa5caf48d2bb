// The reference's wire format on the device (fphe_wire_lengths / _encode / _decode).
#pragma once
#include "mont_dev.h"

namespace {
using namespace fphe;

// ---- wire format: bincode(serde(rug::Integer)) records (fate_utils pickles) ------------
// A reference Ciphertext / Plaintext serializes (bincode 1.3 fixint, little endian) as
//   i32 radix | u64 len | len ASCII chars ("-"? + digits, no leading zeros) | i32 exp
// (BInt is a newtype over rug::Integer, math/src/rug/mod.rs:11; rug's serde writes an
// Integer as the struct {radix, value}; pickles are bincode::serialize, paillier.rs:219-226).
// rug picks the radix per value: decimal when the magnitude has at most 32 significant bits,
// lowercase hex otherwise (rug 1.20 integer/serde.rs; unpinned).  mag is
// element-major LSF uint32 [count][L] (fphe_export_signed).
__device__ __forceinline__ u32 dec_digits(u32 w) {
  u32 d = 1;
  for (u64 p = 10; p <= w; p *= 10) ++d;
  return d;
}

// digits and radix of one magnitude
__device__ __forceinline__ u32 wire_digits(const u32* __restrict__ m, u32 L, u32& radix) {
  int k = (int)L - 1;
  while (k > 0 && m[k] == 0) --k;
  const u32 w = m[k];
  if (k == 0) {
    radix = 10;
    return dec_digits(w);
  }
  radix = 16;
  const u32 nib = (32u - (u32)__builtin_clz(w) + 3u) / 4u;
  return (u32)k * 8u + nib;
}

__global__ __launch_bounds__(256) void k_wire_lengths(const u32* __restrict__ mag, const u8* __restrict__ neg, u32 L,
                                                      size_t count, int64_t* __restrict__ rec_len,
                                                      u8* __restrict__ radix) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  u32 rdx;
  const u32 nd = wire_digits(mag + e * L, L, rdx);
  rec_len[e] = 4 + 8 + 4 + (int64_t)(neg[e] ? 1 : 0) + (int64_t)nd;
  radix[e] = (u8)rdx;
}

// one thread per (element, 32-bit word): for a hex record the word's 8 nibbles are digit
// positions 8k .. 8k+7 from the least significant end; word 0's thread also writes the
// header, the sign and the exponent, and all digits of a decimal (<= 32-bit) record.
__global__ __launch_bounds__(256) void k_wire_encode(const u32* __restrict__ mag, const u8* __restrict__ neg,
                                                     const int32_t* __restrict__ exp, u32 L, size_t count,
                                                     const int64_t* __restrict__ rec_off,
                                                     const int64_t* __restrict__ rec_len, const u8* __restrict__ radix,
                                                     u8* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= count * L) return;
  const size_t e = t / L;
  const u32 k = (u32)(t % L);
  const u32* m = mag + e * L;
  const u32 sg = neg[e] ? 1u : 0u;
  const u32 digits = (u32)(rec_len[e] - 16 - sg);
  const u32 rdx = radix[e];
  if (rdx == 10 && k != 0) return;
  if (rdx != 10 && 8u * k >= digits) return;
  u8* r = out + rec_off[e];
  u8* d = r + 12 + sg;
  if (k == 0) {
    const uint64_t len = digits + sg;
    r[0] = (u8)rdx; r[1] = 0; r[2] = 0; r[3] = 0;
    for (int b = 0; b < 8; ++b) r[4 + b] = (u8)(len >> (8 * b));
    if (sg) r[12] = '-';
    const u32 x = (u32)exp[e];
    u8* ex = r + 12 + sg + digits;
    for (int b = 0; b < 4; ++b) ex[b] = (u8)(x >> (8 * b));
    if (rdx == 10) {
      u32 w = m[0];
      for (u32 j = 0; j < digits; ++j) {
        d[digits - 1 - j] = (u8)('0' + w % 10u);
        w /= 10u;
      }
      return;
    }
  }
  const u32 w = m[k];
  for (u32 i = 0; i < 8; ++i) {
    const u32 j = 8u * k + i;
    if (j >= digits) break;
    const u32 nib = (w >> (4 * i)) & 15u;
    d[digits - 1 - j] = (u8)(nib < 10 ? '0' + nib : 'a' + nib - 10);
  }
}

// digit strings back to magnitude words (radix 16: one thread per word; radix 10 with at
// most 19 digits: word 0's thread writes words 0 and 1; other radixes are parsed on the
// host).  err bit 0: a character that is not a digit of the radix, bit 1: a value wider
// than L words.
__global__ __launch_bounds__(256) void k_wire_decode(const u8* __restrict__ buf, const int64_t* __restrict__ dig_off,
                                                     const int32_t* __restrict__ dig_len, const int32_t* __restrict__ radix,
                                                     u32 L, size_t count, u32* __restrict__ mag,
                                                     int32_t* __restrict__ err) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= count * L) return;
  const size_t e = t / L;
  const u32 k = (u32)(t % L);
  const int64_t off = dig_off[e];
  const u32 len = (u32)dig_len[e];
  u32 bad = 0;
  if (radix[e] == 10) {
    if (k == 0) {
      u64 v = 0;
      for (u32 i = 0; i < len; ++i) {
        const u32 ch = buf[off + i];
        if (ch < '0' || ch > '9') { bad |= 1u; break; }
        v = v * 10u + (ch - '0');
      }
      mag[e * L] = (u32)v;
      if (L > 1) mag[e * L + 1] = (u32)(v >> 32);
      else if (v >> 32) bad |= 2u;
    } else if (k > 1) {
      mag[e * L + k] = 0;
    }
    if (bad) atomicOr(err, (int32_t)bad);
    return;
  }
  u32 w = 0;
  for (u32 i = 0; i < 8; ++i) {
    const u32 j = 8u * k + i;
    if (j >= len) break;
    const u32 ch = buf[off + len - 1 - j];
    u32 v;
    if (ch >= '0' && ch <= '9') v = ch - '0';
    else if (ch >= 'a' && ch <= 'f') v = ch - 'a' + 10;
    else if (ch >= 'A' && ch <= 'F') v = ch - 'A' + 10;
    else { v = 0; bad |= 1u; }
    w |= v << (4 * i);
  }
  mag[e * L + k] = w;
  if (k == L - 1) {  // digits past the top word must be zeros
    for (u32 j = 8u * L; j < len; ++j) {
      const u32 ch = buf[off + len - 1 - j];
      if (ch != '0') { bad |= 2u; break; }
    }
  }
  if (bad) atomicOr(err, (int32_t)bad);
}
}  // namespace
