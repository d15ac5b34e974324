// enc_common.h -- what the encoders' forward (encoder.hip) and backward (encoder_grad.hip) kernels share: the operand
// precisions (fp32 = three bf16 pieces), the weight fragment store and the tile geometry of k_enc_conv.
#pragma once

#include "mfma_conv.h"

namespace dvc {

constexpr int enc_pieces(int dtype) { return dtype == DVC_F32 ? 3 : 1; }

// f(T{}, std::integral_constant<int, NP>{}) with the operand type and piece count of a DVC_* dtype
template <typename F> inline void enc_with_precision(int dtype, F &&f) {
    if (dtype == DVC_F32) f(bf16_t{}, std::integral_constant<int, 3>{});
    else if (dtype == DVC_BF16) f(bf16_t{}, std::integral_constant<int, 1>{});
    else f(f16_t{}, std::integral_constant<int, 1>{});
}

// one accumulator step: NP = 1 one product; NP = 3 the products a_i b_j with i + j <= 2, smallest first
template <typename T, int NP>
__device__ __forceinline__ f32x4 enc_mma(const u32x4 (&a)[NP], const u32x4 (&b)[NP], f32x4 d) {
    if constexpr (NP == 3) {
        d = mma16<T>(a[2], b[0], d);
        d = mma16<T>(a[1], b[1], d);
        d = mma16<T>(a[0], b[2], d);
        d = mma16<T>(a[1], b[0], d);
        d = mma16<T>(a[0], b[1], d);
    }
    return mma16<T>(a[0], b[0], d);
}

// eight fp32 values -> NP operand registers: each piece is the 16-bit rounding of what the pieces before it left
// (the subtractions are exact)
template <typename T, int NP> __device__ __forceinline__ void enc_split8(const float (&f)[8], u32x4 (&bf)[NP]) {
    unsigned p[NP][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = f[2 * j], b = f[2 * j + 1];
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            const unsigned h = pack2_16<T>(a, b);
            p[pc][j] = h;
            a -= bits16_to_f32<T>(h);
            b -= bits16_to_f32<T>(h >> 16);
        }
    }
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) bf[pc] = u32x4{p[pc][0], p[pc][1], p[pc][2], p[pc][3]};
}

// weight v -> value j of lane l of fragment fr: NP pieces, one kFragBytes behind the other
template <typename T, int NP>
__device__ __forceinline__ void enc_pack_store(unsigned char *out, int fr, int l, int j, float v) {
    T *dst = reinterpret_cast<T *>(out + (long long)fr * NP * kFragBytes) + l * 8 + j;
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) {
        T h;
        StoreT<T>::store(&h, v);
        dst[pc * (kFragBytes / 2)] = h;
        v -= StoreT<T>::load(&h);
    }
}

constexpr int EN_TH = DVC_ENC_TH, EN_TD = DVC_ENC_TD;

// column groups per wave = output box extent along W
constexpr int enc_tw(int taps, int stride) { return taps == 27 && stride == 2 ? 2 : DVC_ENC_TW; }
// output tiles per workgroup and the packed tile count (a multiple of it)
inline int enc_ntw(int taps, int cout) {
    const int nt = (cout + 15) / 16;
    return nt == 1 ? 1 : (nt == 2 || taps == 27) ? 2 : 4;
}
inline int enc_ntp(int taps, int cout) {
    const int ntw = enc_ntw(taps, cout);
    return ((cout + 15) / 16 + ntw - 1) / ntw * ntw;
}
inline int enc_out_extent(int n, int stride) { return (n - 1) / stride + 1; }
inline int enc_nch(int taps, int cin) { return taps == 27 ? cin / 8 : (cin + 31) / 32; }
inline int enc_ksteps(int taps) { return taps == 27 ? 7 : 1; }

}  // namespace dvc
