// Host-only core of the weight and filter packers (conv_split.hip,
// unit_split.hip, edge_split.hip): the per-row scaling exponent, the operand
// splits, and the fragment writer of the MFMA weight images.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

namespace rave {

// Power-of-two row exponent: max |w * 2^e| in [8, 16) (e = 0 for an all-zero row).
inline int row_exponent(double amax) {
    if (!(amax > 0.0)) return 0;
    int e = (int)std::floor(std::log2(16.0 / amax));
    while (std::ldexp(amax, e) >= 16.0) --e;
    while (std::ldexp(amax, e) < 8.0) ++e;
    return e;
}

// fp32 -> bf16, round to nearest even (finite weights), and back (exact)
inline uint16_t bf16_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_value(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// split-f16 pair of an (already row-scaled) value: hi = f16(v), lo = f16((v - hi) * 2^11)
inline void split_f16(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)((v - (float)hi) * 2048.0f);
}

// Packed-image arithmetic of the MFMA kernels: a fragment is 64 lanes x 8
// values of one K-step and 32-row block, held in pack_planes(mode) consecutive
// 1 KB slots.
enum PackMode { kPackSplit16 = 0, kPackF32 = 1, kPackBf16x3 = 2 };
constexpr int pack_planes(int mode) { return mode == kPackBf16x3 ? 3 : 2; }
// floats of `fragments` fragments of `planes` slots, plus `tail` trailing floats (row scales)
constexpr int64_t packed_floats(int64_t fragments, int planes, int64_t tail) {
    return fragments * planes * 256 + tail;
}

// Writes value v (lane, element e of 8) of fragment `fragment` into its slots:
//   split16: f16 planes hi | lo of the row-scaled v;
//   fp32:    floats 0-3 of a lane in slot 0, 4-7 in slot 1;
//   bf16x3:  bf16 planes hi | lo | mid with v == hi + mid + lo exactly.
inline void put_fragment(float* packed, int64_t fragment, int mode, int lane, int e, float v) {
    const int64_t slot = fragment * pack_planes(mode);
    if (mode == kPackBf16x3) {
        uint16_t* bp = reinterpret_cast<uint16_t*>(packed) + slot * 512;
        const uint16_t h = bf16_bits(v);
        const float r = v - bf16_value(h);
        const uint16_t md = bf16_bits(r);
        bp[lane * 8 + e] = h;
        bp[1024 + lane * 8 + e] = md;
        bp[512 + lane * 8 + e] = bf16_bits(r - bf16_value(md));
    } else if (mode == kPackF32) {
        packed[slot * 256 + (e >> 2) * 256 + lane * 4 + (e & 3)] = v;
    } else {
        _Float16* hi = reinterpret_cast<_Float16*>(packed) + slot * 512;
        split_f16(v, hi[lane * 8 + e], hi[512 + lane * 8 + e]);
    }
}

}  // namespace rave
