// gru.hip -- one axis pass of the update block's SepConvGRU3D, fused (round 7)
// (reference: SepConvGRU3D.forward, src/core/update.py:167-199; hidden 96, input 147 in BasicUpdateBlock,
// update.py:283-297).  Per axis a in (h, w, d), with conv_*_a a 5-tap 1-D convolution zero-padded by 2 along a:
//     hx = cat[h, x];  z = sigmoid(conv_z(hx));  r = sigmoid(conv_r(hx))
//     q  = tanh(conv_q(cat[r h, x]));  h' = (1 - z) h + z q
//
// k_sep_gru_pass.  A workgroup (four waves, one per SIMD) owns S = DVC_GRU_SEG output positions along the conv axis of
// 16 neighbouring lines (a line = the voxels that differ only in the conv-axis coordinate; neighbours are the next
// lines in memory, so for the h and w passes 16 lines are 64 contiguous bytes of every channel).  The pass is an
// implicit GEMM over K = 5 taps x 256 padded input channels (96 hidden, then the input padded to 160), walked in
// eight chunks of 32 channels:
//   stage    every thread loads one voxel's 32 channels of the chunk (fp32, coalesced over the lines; over the
//            positions for the d pass) and writes them as one 64-byte row [voxel][32 ch] of 16-bit values to LDS,
//            S + 8 positions x 16 lines; out-of-volume positions, missing lines and padding channels are zeros.
//            The next chunk's loads are in flight under the current chunk's MFMAs.
//   phase 1  z and r (N = 192, twelve 16-channel tiles) for S + 4 positions on v_mfma_f32_16x16x32: the weights are
//            the A operand (one 1 KB fragment per (chunk, tap, tile), read straight from the packed buffer, L2), the
//            voxels the B operand (16 lines of one position per MFMA; tap t reads the LDS rows of position p + t).
//            Wave w owns positions 3 w .. 3 w + 2 with all twelve tiles: 144 accumulator registers.
//   phase 2  q (N = 96) for the S centre positions, over chunks of cat[r h, x]: the owner of a position writes
//            r * h of its positions into the chunk buffer (r from its registers, h reloaded in fp32; h is read as 0
//            outside the volume, so r h is exactly zero there, as the reference's padding of cat[r h, x]); the x
//            chunks are staged as in phase 1.  A wave computes q at those of its phase-1 positions that are
//            centre positions, so z never leaves its registers (waves 0 and 3 hold one such position, 1 and 2
//            three: the price of keeping z, r and q out of LDS and memory).
//   blend    tanh, (1 - z) h + z q with h reloaded in fp32, stored to h_out (never the buffer being read).
// z, r, q and hx never reach memory; no atomics; no allocation or synchronisation on the host.
//
// Precisions.  T = bf16 / fp16, NP = 1: operands rounded once, fp32 accumulation, gates and blend in fp32.
// fp32 (T = bf16, NP = 2): every operand is split into bf16 hi + lo, three MFMAs per step
// (w_hi x_hi + w_hi x_lo + w_lo x_hi), as the fp32 convc1 consumers do.
//
// LDS: 256 rows x 80 bytes (64 + 16: the 16 lanes of a b128 read land on distinct banks) per piece: 20 KB, 40 KB
// for fp32.
#include "mfma_conv.h"

namespace dvc {

constexpr int GRU_S = DVC_GRU_SEG;      // output positions per workgroup
constexpr int GRU_HID = DVC_GRU_HIDDEN; // hidden channels
constexpr int GRU_NCH = 8;              // chunks of 32 padded input channels (3 hidden + 5 input)
constexpr int GRU_UNITS1 = GRU_NCH * 5 * 2;   // phase-1 weight units (chunk, tap, half) of six fragments
constexpr int GRU_UNITS2 = GRU_NCH * 5;       // phase-2 weight units (chunk, tap)
constexpr int GRU_FRAGS = (GRU_UNITS1 + GRU_UNITS2) * 6;   // 1 KB fragments per piece

struct GruArgs {
    const float *h, *x;
    const unsigned char *w;   // packed weights of this axis (dvc_gru_pack), then 288 fp32 biases (z, r, q)
    float *out;
    float *save;              // SAVE: z, r, q (after tanh) of the centre positions, three (B, 96, H, W, D) tensors in a row
    long long HWD, pstride;   // channel stride; stride of one step along the conv axis
    int B, Cx, H, W, D, axis, len, nlines, per_b;
};

__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <typename T, int NP, bool SAVE>
__global__ __launch_bounds__(256, 1) void k_sep_gru_pass(GruArgs A) {
    constexpr int S = GRU_S, PB = (S + 4) / 4, ROWB = kRowBytes, PIECE = 16 * (S + 8) * ROWB;
    static_assert(S == 8, "256 threads stage (S + 8) positions x 16 lines, one voxel each");
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * PIECE];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nlg = (A.nlines + 15) / 16;
    const int lg = (int)(blockIdx.x % (unsigned)nlg), seg0 = (int)(blockIdx.x / (unsigned)nlg) * S;
    const long long HWD = A.HWD;

    // the voxel this thread stages: consecutive lanes walk the contiguous direction
    const int sline = A.axis == 2 ? tid >> 4 : tid & 15;
    const int sp = A.axis == 2 ? tid & 15 : tid >> 4;
    int sb;
    long long soff;
    bool sok = gru_line(A, lg * 16 + sline, sb, soff);
    const int spos = seg0 - 4 + sp;
    sok = sok && spos >= 0 && spos < A.len;
    if (!sok) { sb = 0; soff = 0; } else soff += (long long)spos * A.pstride;
    const float *sh = A.h + (long long)sb * GRU_HID * HWD + soff;
    const float *sx = A.x + (long long)sb * A.Cx * HWD + soff;
    unsigned char *srow = smem + (sp * 16 + sline) * ROWB;

    // the line of this lane's MFMA column
    int mb;
    long long moff;
    const bool mok = gru_line(A, lg * 16 + m16, mb, moff);
    const float *mh = A.h + (long long)mb * GRU_HID * HWD + moff;
    float *mo = A.out + (long long)mb * GRU_HID * HWD + moff;
    float *ms = SAVE ? A.save + (long long)mb * GRU_HID * HWD + moff : nullptr;
    const long long NS = (long long)A.B * GRU_HID * HWD;   // one saved tensor

    const unsigned char *w1 = A.w + lane * 16;
    const unsigned char *w2 = w1 + (long long)GRU_UNITS1 * 6 * NP * kFragBytes;
    const float *bias = reinterpret_cast<const float *>(A.w + (long long)GRU_FRAGS * NP * kFragBytes);

    float st[32];   // staging registers: one voxel's 32 channels, or the owner's h values of an r h chunk
    auto stage_load = [&](int c) __attribute__((always_inline)) {   // chunk c of cat[h, x]
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int kp = 32 * c + k;
            const bool ok = sok && kp < GRU_HID + A.Cx;
            const float *p = kp < GRU_HID ? sh + (long long)kp * HWD : sx + (long long)(kp - GRU_HID) * HWD;
            st[k] = ok ? *p : 0.0f;
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) { stage_row<T, NP>(st, srow, PIECE); };

    u32x4 wc[6][NP], wn[6][NP];
    // the MFMAs of one staged chunk: five taps x NH halves of six tiles; pv[i] = position i of this wave takes part
    auto chunk_mfma = [&](auto nh_c, f32x4 (&acc)[6 * decltype(nh_c)::value][PB], const unsigned char *wb, int &u,
                          int nunits, const bool (&pv)[PB]) __attribute__((always_inline)) {
        constexpr int NH = decltype(nh_c)::value;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            u32x4 bf[PB][NP];
#pragma unroll
            for (int i = 0; i < PB; ++i)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
                    bf[i][pc] = *reinterpret_cast<const u32x4 *>(smem + pc * PIECE +
                                                                 ((PB * wave + i + t) * 16 + m16) * ROWB + h4 * 16);
#pragma unroll
            for (int hf = 0; hf < NH; ++hf) {
                ++u;
                load_frags(wb, u, nunits, 6, wn);   // the next unit's fragments, in flight under this unit's MFMAs
#pragma unroll
                for (int tl = 0; tl < 6; ++tl)
#pragma unroll
                    for (int i = 0; i < PB; ++i)
                        if (pv[i]) acc[hf * 6 + tl][i] = mma_step<T, NP>(wc[tl], bf[i], acc[hf * 6 + tl][i]);
#pragma unroll
                for (int tl = 0; tl < 6; ++tl)
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc) wc[tl][pc] = wn[tl][pc];
            }
        }
    };

    // ---------------- phase 1: z and r at positions seg0 - 2 + (PB wave + i) ----------------
    f32x4 zg[6][PB], rg[6][PB];
    {
        f32x4 acc[12][PB];
#pragma unroll
        for (int t = 0; t < 12; ++t)
#pragma unroll
            for (int i = 0; i < PB; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool all[PB] = {true, true, true};
        int u = 0;
        load_frags(w1, 0, GRU_UNITS1, 6, wc);
        stage_load(0);
#pragma unroll 1
        for (int c = 0; c < GRU_NCH; ++c) {
            __syncthreads();   // the previous chunk's reads are done
            stage_write();
            __syncthreads();
            if (c + 1 < GRU_NCH) stage_load(c + 1);
            chunk_mfma(std::integral_constant<int, 2>{}, acc, w1, u, GRU_UNITS1, all);
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int o0 = 16 * t + 4 * h4;
#pragma unroll
            for (int i = 0; i < PB; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    zg[t][i][k] = gru_sigmoid(acc[t][i][k] + bias[o0 + k]);
                    rg[t][i][k] = gru_sigmoid(acc[6 + t][i][k] + bias[GRU_HID + o0 + k]);
                }
        }
    }

    // ---------------- phase 2: q at the centre positions among them ----------------
    bool pv[PB];
    int ppos[PB];   // volume position of this wave's position i
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int q = PB * wave + i - 2;
        pv[i] = q >= 0 && q < S;
        ppos[i] = seg0 + q;
    }
    if constexpr (SAVE) {   // r leaves now: its registers are free after the last r h chunk
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if (!(pv[i] && mok && ppos[i] < A.len)) continue;
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    ms[NS + (long long)(16 * t + 4 * h4 + k) * HWD + (long long)ppos[i] * A.pstride] = rg[t][i][k];
        }
    }
    f32x4 acq[6][PB];
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int i = 0; i < PB; ++i) acq[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    int u = 0;
    load_frags(w2, 0, GRU_UNITS2, 6, wc);
    // h of this lane's 2 x PB x 4 values of r h chunk c (tiles 2c, 2c + 1): zero outside the volume
    auto rh_load = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const bool ok = mok && ppos[i] >= 0 && ppos[i] < A.len;
                const float *p = mh + (long long)(16 * (2 * c + tt) + 4 * h4) * HWD + (ok ? (long long)ppos[i] * A.pstride : 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) st[(tt * PB + i) * 4 + k] = ok ? p[(long long)k * HWD] : 0.0f;
            }
    };
    auto rh_write = [&](auto c_c) __attribute__((always_inline)) {
        constexpr int c = decltype(c_c)::value;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = rg[2 * c + tt][i][k] * st[(tt * PB + i) * 4 + k];
                unsigned h0, l0, h1, l1;
                split2<T, NP>(v[0], v[1], h0, l0);
                split2<T, NP>(v[2], v[3], h1, l1);
                unsigned char *d = smem + ((PB * wave + i + 2) * 16 + m16) * ROWB + tt * 32 + h4 * 8;
                *reinterpret_cast<u32x2 *>(d) = u32x2{h0, h1};
                if constexpr (NP == 2) *reinterpret_cast<u32x2 *>(d + PIECE) = u32x2{l0, l1};
            }
    };
    auto rh_chunk = [&](auto c_c) __attribute__((always_inline)) {
        constexpr int c = decltype(c_c)::value;
        __syncthreads();
        rh_write(c_c);
        __syncthreads();
        if constexpr (c + 1 < 3) rh_load(c + 1);
        else stage_load(3);
        chunk_mfma(std::integral_constant<int, 1>{}, acq, w2, u, GRU_UNITS2, pv);
    };
    rh_load(0);
    rh_chunk(std::integral_constant<int, 0>{});
    rh_chunk(std::integral_constant<int, 1>{});
    rh_chunk(std::integral_constant<int, 2>{});
#pragma unroll 1
    for (int c = 3; c < GRU_NCH; ++c) {
        __syncthreads();
        stage_write();
        __syncthreads();
        if (c + 1 < GRU_NCH) stage_load(c + 1);
        chunk_mfma(std::integral_constant<int, 1>{}, acq, w2, u, GRU_UNITS2, pv);
    }

    // ---------------- blend: h' = (1 - z) h + z tanh(q) ----------------
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        if (!(pv[i] && mok && ppos[i] < A.len)) continue;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int o0 = 16 * t + 4 * h4;
            const long long base = (long long)o0 * HWD + (long long)ppos[i] * A.pstride;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float hv = mh[base + (long long)k * HWD];
                const float q = tanhf(acq[t][i][k] + bias[2 * GRU_HID + o0 + k]);
                const float z = zg[t][i][k];
                mo[base + (long long)k * HWD] = (1.0f - z) * hv + z * q;
                if constexpr (SAVE) {
                    ms[base + (long long)k * HWD] = z;
                    ms[2 * NS + base + (long long)k * HWD] = q;
                }
            }
        }
    }
}

// Packed weights of one axis: fragment f = (chunk c, tap t, tile) of phase 1 ([c][t][12 tiles: z 0..5, r 0..5]), then of
// phase 2 ([c][t][6 tiles of q]); each fragment NP pieces of [lane][8] 16-bit values, lane l element j = weight
// [o = 16 tile + (l & 15)][padded input channel 32 c + 8 (l >> 4) + j][t]; then the 288 biases.
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_gru_pack(const float *__restrict__ wz, const float *__restrict__ wr,
                                                  const float *__restrict__ wq, const float *__restrict__ bz,
                                                  const float *__restrict__ br, const float *__restrict__ bq,
                                                  unsigned char *__restrict__ out, int Cx) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= GRU_FRAGS * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const float *w;
    int tile, ct;
    if (fr < GRU_UNITS1 * 6) {
        const int t12 = fr % 12;
        ct = fr / 12;
        w = t12 < 6 ? wz : wr;
        tile = t12 % 6;
    } else {
        const int f2 = fr - GRU_UNITS1 * 6;
        ct = f2 / 6;
        w = wq;
        tile = f2 % 6;
    }
    const int c = ct / 5, t = ct % 5;
    const int o = 16 * tile + (l & 15), kp = 32 * c + 8 * (l >> 4) + j, cin = GRU_HID + Cx;
    const float v = kp < cin ? w[((long long)o * cin + kp) * 5 + t] : 0.0f;
    pack_store<T, NP>(out, fr, l, j, v);
    if (e < 3 * GRU_HID) {
        float *b = reinterpret_cast<float *>(out + (long long)GRU_FRAGS * NP * kFragBytes);
        b[e] = e < GRU_HID ? bz[e] : e < 2 * GRU_HID ? br[e - GRU_HID] : bq[e - 2 * GRU_HID];
    }
}

size_t gru_packed_bytes(int dtype) {
    return (size_t)GRU_FRAGS * pieces_of(dtype) * kFragBytes + 3 * GRU_HID * sizeof(float);
}

hipError_t launch_gru_pack(const float *wz, const float *wr, const float *wq, const float *bz, const float *br,
                           const float *bq, void *packed, int Cx, int dtype, hipStream_t s) {
    const unsigned blocks = GRU_FRAGS * 512 / 256;
    unsigned char *out = static_cast<unsigned char *>(packed);
    with_precision(dtype, [&](auto t, auto np) {
        k_gru_pack<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(wz, wr, wq, bz, br, bq, out, Cx);
    });
    return hipGetLastError();
}

// host entry: arguments validated by dvc_sep_gru_pass / dvc_sep_gru_pass_save (capi.hip); save = nullptr: inference
hipError_t launch_sep_gru_pass(const float *h, const float *x, const void *packed, float *h_out, float *save, int B,
                               int Cx, int H, int W, int D, int axis, int dtype, hipStream_t s) {
    GruArgs A;
    A.h = h; A.x = x; A.w = static_cast<const unsigned char *>(packed); A.out = h_out; A.save = save;
    A.B = B; A.Cx = Cx; A.H = H; A.W = W; A.D = D; A.axis = axis;
    A.HWD = (long long)H * W * D;
    A.len = axis == 0 ? H : axis == 1 ? W : D;
    A.pstride = axis == 0 ? (long long)W * D : axis == 1 ? D : 1;
    A.per_b = (int)(A.HWD / A.len);
    A.nlines = B * A.per_b;
    const unsigned grid = (unsigned)((A.nlines + 15) / 16) * (unsigned)((A.len + GRU_S - 1) / GRU_S);
    with_precision(dtype, [&](auto t, auto np) {
        if (save) k_sep_gru_pass<decltype(t), decltype(np)::value, true><<<grid, 256, 0, s>>>(A);
        else k_sep_gru_pass<decltype(t), decltype(np)::value, false><<<grid, 256, 0, s>>>(A);
    });
    return hipGetLastError();
}

}  // namespace dvc
