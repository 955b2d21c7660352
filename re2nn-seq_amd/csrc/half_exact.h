// Which f32 values the 16-bit image of a block may hold (layout.hip.h, half_image_kernel): exactly the ones an IEEE f16 represents
// as a NORMAL number or a zero -- (float)(half)x == x, and no f16 subnormal (|x| >= 2^-14), so the result never depends on a
// denormal mode.  Bit arithmetic on the f32 pattern, no f16 type: the same function on the host (tests/test_half_eligibility.py
// holds it to a table of values) and in the device-side reduction.  No HIP header needed.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FARNN_HALF_HD __host__ __device__
#else
#define FARNN_HALF_HD
#endif

namespace farnn {

FARNN_HALF_HD inline uint32_t f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

// +0 and -0 pass (0 + W and the f16 round trip both keep the sign); inf and nan do not
FARNN_HALF_HD inline bool half_exact(float x) {
    const uint32_t u = f32_bits(x), e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e == 0) return m == 0;                           // a zero; an f32 subnormal is far below 2^-14
    if (e < 127 - 14 || e > 127 + 15) return false;      // below the smallest normal f16, above the largest (inf / nan: e = 255)
    return (m & 0x1fffu) == 0;                           // ten mantissa bits
}

// the f16 pattern of a value half_exact() passed
FARNN_HALF_HD inline uint16_t half_bits_exact(float x) {
    const uint32_t u = f32_bits(x), e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
    if (e == 0) return s;
    return (uint16_t)(s | ((e - 127 + 15) << 10) | (m >> 13));
}

}  // namespace farnn
