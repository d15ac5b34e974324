// mfma_conv.h -- what the update block's implicit-GEMM kernels on v_mfma_f32_16x16x32 share (gru.hip, conv3.hip):
// the weights are the A operand, packed as 1 KB fragments; the voxels are the B operand, staged to LDS as rows of 32
// channels.  T = bf16 / fp16 with NP = 1 piece: operands rounded once, fp32 accumulation.  fp32 is T = bf16 with
// NP = 2 pieces: every operand is split into bf16 hi + lo and a step takes three products.
#pragma once

#include "common.h"

#include <type_traits>

namespace dvc {

// one piece of a weight fragment: [64 lanes][8] 16-bit values, lane l's eight values its A operand of one MFMA
constexpr int kFragBytes = 1024;
// pitch of an LDS row of 32 16-bit channels: 64 + 16 bytes, so the 16 lanes of a b128 read land on distinct banks
constexpr int kRowBytes = 80;

constexpr int pieces_of(int dtype) { return dtype == DVC_F32 ? 2 : 1; }

// f(T{}, std::integral_constant<int, NP>{}) with the operand type and piece count of a DVC_* dtype
template <typename F> inline void with_precision(int dtype, F &&f) {
    if (dtype == DVC_F32) f(bf16_t{}, std::integral_constant<int, 2>{});
    else if (dtype == DVC_BF16) f(bf16_t{}, std::integral_constant<int, 1>{});
    else f(f16_t{}, std::integral_constant<int, 1>{});
}

template <typename T> __device__ __forceinline__ f32x4 mma16(u32x4 a, u32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mma16<bf16_t>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}
template <> __device__ __forceinline__ f32x4 mma16<f16_t>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
}

// one accumulator step: NP = 1 one product, NP = 2 the three products of the hi + lo split (w_lo x_hi, w_hi x_lo,
// w_hi x_hi, in this order)
template <typename T, int NP>
__device__ __forceinline__ f32x4 mma_step(const u32x4 (&a)[NP], const u32x4 (&b)[NP], f32x4 d) {
    if constexpr (NP == 2) {
        d = mma16<T>(a[1], b[0], d);
        d = mma16<T>(a[0], b[1], d);
    }
    return mma16<T>(a[0], b[0], d);
}

// two fp32 values -> one dword of 16-bit hi pieces and (NP = 2) one of lo pieces
template <typename T, int NP> __device__ __forceinline__ void split2(float a, float b, unsigned &hi, unsigned &lo) {
    hi = pack2_16<T>(a, b);
    lo = 0u;
    if constexpr (NP == 2) lo = pack2_16<T>(a - bits16_to_f32<T>(hi), b - bits16_to_f32<T>(hi >> 16));
}

// 32 channels of one voxel -> its 64-byte LDS row of hi pieces and (NP = 2) the lo row piece_bytes further on
template <typename T, int NP>
__device__ __forceinline__ void stage_row(const float (&v)[32], unsigned char *row, int piece_bytes) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split2<T, NP>(v[8 * o + 2 * j], v[8 * o + 2 * j + 1], hi[j], lo[j]);
        *reinterpret_cast<u32x4 *>(row + o * 16) = u32x4{hi[0], hi[1], hi[2], hi[3]};
        if constexpr (NP == 2)
            *reinterpret_cast<u32x4 *>(row + piece_bytes + o * 16) = u32x4{lo[0], lo[1], lo[2], lo[3]};
    }
}

// This lane's share of the first N fragments of weight unit u, a unit being per_unit fragments of NP pieces;
// wb = packed buffer + 16 lane.  u is clamped to the last unit, so the prefetch after the last step stays in bounds.
template <int N, int NP>
__device__ __forceinline__ void load_frags(const unsigned char *wb, int u, int nunits, int per_unit,
                                           u32x4 (&wf)[N][NP]) {
    const unsigned char *p = wb + (long long)(u < nunits ? u : nunits - 1) * per_unit * NP * kFragBytes;
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) wf[t][pc] = *reinterpret_cast<const u32x4 *>(p + (t * NP + pc) * kFragBytes);
}

// pack kernels: element e of the packed fragments -> fragment fr, lane l, value j of the lane
__device__ __forceinline__ void frag_elem(int e, int &fr, int &l, int &j) {
    j = e & 7;
    l = (e >> 3) & 63;
    fr = e >> 9;
}
// weight v -> value j of lane l of fragment fr: the hi piece and (NP = 2) the lo piece v - hi behind it
template <typename T, int NP>
__device__ __forceinline__ void pack_store(unsigned char *out, int fr, int l, int j, float v) {
    T *dst = reinterpret_cast<T *>(out + (long long)fr * NP * kFragBytes) + l * 8 + j;
    T hi;
    StoreT<T>::store(&hi, v);
    dst[0] = hi;
    if constexpr (NP == 2) StoreT<T>::store(dst + kFragBytes / 2, v - StoreT<T>::load(&hi));
}

// packed tiles of a 3 x 3 x 3 layer's output channel count: 4 FULL + SHARED of the k_conv3_mfma instance that runs it
inline int conv3_tiles(int cout) {
    const int n = (cout + 15) / 16;
    return n <= 2 ? n : n <= 4 ? 4 : n == 5 ? 5 : 8;
}

// Element e of a 3 x 3 x 3 layer's packed weights (k_conv3_pack, k_conv3_pack_dgrad): fragment ((chunk c, tap t = (kh 3
// + kw) 3 + kd), tile), NP pieces of [lane][8] 16-bit values each: lane l element j = weight(o = 16 tile + (l & 15),
// input channel 32 c + 8 (l >> 4) + j, t), zero where o >= cout or the channel >= cin; then 16 nt float32 biases
// bias(o) (zero past cout).
template <typename T, int NP, typename WF, typename BF>
__device__ __forceinline__ void conv3_pack_elem(int e, unsigned char *out, int cin, int cout, int nch, int nt,
                                                WF weight, BF bias) {
    const int nfr = nch * 27 * nt;
    if (e >= nfr * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int tile = fr % nt, ct = fr / nt, c = ct / 27, t = ct - 27 * c;
    const int o = 16 * tile + (l & 15), kp = 32 * c + 8 * (l >> 4) + j;
    pack_store<T, NP>(out, fr, l, j, o < cout && kp < cin ? weight(o, kp, t) : 0.0f);
    if (e < 16 * nt) reinterpret_cast<float *>(out + (long long)nfr * NP * kFragBytes)[e] = e < cout ? bias(e) : 0.0f;
}

// workgroup bid of a (B, nth, ntw, ntd) grid of TH x TW x TD output boxes -> batch element and box origin
__device__ __forceinline__ void box_of_block(unsigned bid, int nth, int ntw, int ntd, int TH, int TW, int TD, int &b,
                                             int &h0, int &w0, int &d0) {
    d0 = (int)(bid % (unsigned)ntd) * TD;
    bid /= (unsigned)ntd;
    w0 = (int)(bid % (unsigned)ntw) * TW;
    bid /= (unsigned)ntw;
    h0 = (int)(bid % (unsigned)nth) * TH;
    b = (int)(bid / (unsigned)nth);
}

// Line n of a GRU axis pass (a line = the voxels that differ only in the conv-axis coordinate) -> batch element and
// spatial offset of its position 0.  A has nlines, per_b (lines per batch element), axis, W and D.
template <typename Args> __device__ __forceinline__ bool gru_line(const Args &A, int n, int &b, long long &off) {
    b = 0;
    off = 0;
    if (n >= A.nlines) return false;
    b = n / A.per_b;
    const int r = n - b * A.per_b;
    off = A.axis == 0 ? (long long)r : A.axis == 1 ? (long long)(r / A.D) * A.W * A.D + r % A.D : (long long)r * A.D;
    return true;
}

}  // namespace dvc
