// Limb geometry of the reduced-radix engine a TPI runs on (mont27_dev.h): 28 x 37, or 27 x 38 for
// the 4096-bit geometry when built with FPHE_RADIX4=27.  Plain C++: the device code and the
// host-only key-blob builder (key_blob.h) both derive their limb counts from these.
#pragma once

#ifndef FPHE_RADIX4
#define FPHE_RADIX4 28
#endif

namespace fphe {
constexpr int rad_lb(int tpi) { return tpi == 4 ? FPHE_RADIX4 : 28; }
constexpr int rad_ll(int tpi) { return rad_lb(tpi) == 27 ? 38 : 37; }
}  // namespace fphe
