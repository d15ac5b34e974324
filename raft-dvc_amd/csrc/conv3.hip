// conv3.hip -- the update block's plain convolutions on the matrix cores (round 8)
// (reference: BasicMotionEncoder and FlowHead3D / UncertaintyHead3D of BasicUpdateBlock, src/core/update.py:205-348).
//
// k_conv3_mfma.  3 x 3 x 3 convolution, zero padding 1, stride 1, + bias (+ ReLU), on contiguous float32
// (B, C, H, W, D) tensors.  The input is the channel concatenation of src0 (C0 channels) and src1 (C1, may be
// absent); the output is a channel slice [dst_off, dst_off + cout) of a tensor with dst_channels channels.
// An implicit GEMM over K = 27 taps x (C0 + C1 padded to 32-channel chunks) on v_mfma_f32_16x16x32:
//   box      a workgroup (four waves) owns 4 x 4 x 16 output voxels along (H, W, D): sixteen column groups of 16
//            voxels contiguous along D.
//   stage    per 32-channel chunk the 6 x 6 x 18 halo box goes to LDS once as 648 rows [voxel][32 ch] of 16-bit
//            values (80-byte pitch: the 16 lanes of a b128 read land on distinct banks); out-of-volume voxels and
//            padding channels are zeros.  The next chunk's loads are in flight under the current chunk's MFMAs.
//   MFMA     the weights are the A operand (one 1 KB fragment per (chunk, tap, 16-channel tile), read straight
//            from the packed buffer), the voxels the B operand: tap (dh, dw, dd) of column group (bh, bw) reads
//            the rows of voxel (bh + dh, bw + dw, m + dd).
//   split    the waves own OUTPUT TILES, not voxels: wave w owns the FULL tiles w, w + 4, .. at all sixteen column
//            groups, so a weight fragment is fetched by one wave per workgroup.  The SHARED tiles that are left
//            when the tile count is no multiple of four are computed by every wave at its own four column groups
//            (bh = w).  cout 128: FULL 2; 80: FULL 1 + SHARED 1; 32: SHARED 2; 3: SHARED 1.
// Precisions as gru.hip: T = bf16 / fp16, NP = 1: operands rounded once, fp32 accumulation; fp32 (T = bf16,
// NP = 2): bf16 hi + lo pieces, w_hi x_hi + w_hi x_lo + w_lo x_hi.
//
// k_conv7_flow.  encoder.convf1: 3 -> 64 channels, 7 x 7 x 7, zero padding 3, + bias + ReLU.  One K = 32 step per
// (kh, kw) pair, k = 8 ci + kd: the 16-lane group ci of the B operand holds input channel ci's eight consecutive d
// values (the eighth and the fourth group meet zero weights and are zeros).  The 10 x 10 x 22 halo box of the three
// channels sits in LDS in float32; a lane builds its 8-value run in registers from dword reads.  Wave w owns the four
// column groups bh = w with all four output tiles.
//
// No atomics, no allocation or synchronisation on the host.
#include "mfma_conv.h"

namespace dvc {

constexpr int C3_TH = DVC_CONV3_TH, C3_TW = DVC_CONV3_TW, C3_TD = DVC_CONV3_TD;
constexpr int C3_HW = C3_TW + 2, C3_HD = C3_TD + 2;
constexpr int C3_ROWS = (C3_TH + 2) * C3_HW * C3_HD;   // 648 halo voxels
constexpr int C3_PIECE = C3_ROWS * kRowBytes;
constexpr int C3_STAGE = (C3_ROWS + 255) / 256;        // halo rows per thread
static_assert(C3_TH == 4 && C3_TW == 4 && C3_TD == 16, "sixteen column groups of 16 voxels, four per wave");

struct Conv3Args {
    const float *s0, *s1;
    const unsigned char *w;   // packed weights (k_conv3_pack), then 16 x tiles fp32 biases
    float *dst;
    long long HWD;
    int B, C0, C1, H, W, D, dstC, dstOff, cout, relu, nch, nth, ntw, ntd;
};

template <typename T, int NP, int FULL, int SHARED>
__global__ __launch_bounds__(256, 1) void k_conv3_mfma(Conv3Args A) {
    constexpr int NT = 4 * FULL + SHARED;   // packed tiles
    constexpr int NW = FULL + SHARED;       // tiles whose fragments one wave reads
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * C3_PIECE];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b, h0, w0, d0;
    box_of_block(blockIdx.x, A.nth, A.ntw, A.ntd, C3_TH, C3_TW, C3_TD, b, h0, w0, d0);
    const long long HWD = A.HWD;
    const int cin = A.C0 + A.C1;
    const float *s0 = A.s0 + (long long)b * A.C0 * HWD;
    const float *s1 = A.s1 + (long long)b * A.C1 * HWD;   // never read when C1 = 0

    // the halo voxels this thread stages: consecutive lanes walk D
    bool sok[C3_STAGE];
    long long soff[C3_STAGE];
#pragma unroll
    for (int i = 0; i < C3_STAGE; ++i) {
        const int r = tid + 256 * i;
        const int hh = r / (C3_HW * C3_HD), rem = r - hh * (C3_HW * C3_HD), ww = rem / C3_HD, dd = rem - ww * C3_HD;
        const int h = h0 - 1 + hh, w = w0 - 1 + ww, d = d0 - 1 + dd;
        sok[i] = r < C3_ROWS && h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
        soff[i] = sok[i] ? ((long long)h * A.W + w) * A.D + d : 0;
    }

    float st[C3_STAGE][32];
    auto stage_load = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int kp = 32 * c + k;
            const float *p = kp < A.C0 ? s0 + (long long)kp * HWD : s1 + (long long)(kp - A.C0) * HWD;
#pragma unroll
            for (int i = 0; i < C3_STAGE; ++i) st[i][k] = sok[i] && kp < cin ? p[soff[i]] : 0.0f;
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < C3_STAGE; ++i) {
            const int r = tid + 256 * i;
            if (r < C3_ROWS) stage_row<T, NP>(st[i], smem + r * kRowBytes, C3_PIECE);
        }
    };

    // fragment ((chunk, tap), tile, piece): this wave's FULL tiles wave + 4 f, then the SHARED tiles 4 FULL + s
    const unsigned char *wbase = A.w + lane * 16;
    const int nunits = A.nch * 27;
    u32x4 wc[NW][NP], wn[NW][NP];
    auto loadw = [&](int u, u32x4 (&wf)[NW][NP]) __attribute__((always_inline)) {
        const unsigned char *p = wbase + (long long)(u < nunits ? u : nunits - 1) * NT * NP * kFragBytes;
#pragma unroll
        for (int f = 0; f < FULL; ++f)
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                wf[f][pc] = *reinterpret_cast<const u32x4 *>(p + ((wave + 4 * f) * NP + pc) * kFragBytes);
#pragma unroll
        for (int s = 0; s < SHARED; ++s)
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                wf[FULL + s][pc] = *reinterpret_cast<const u32x4 *>(p + ((4 * FULL + s) * NP + pc) * kFragBytes);
    };

    f32x4 accf[FULL > 0 ? FULL : 1][16], accs[SHARED > 0 ? SHARED : 1][4];
#pragma unroll
    for (int f = 0; f < (FULL > 0 ? FULL : 1); ++f)
#pragma unroll
        for (int g = 0; g < 16; ++g) accf[f][g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < (SHARED > 0 ? SHARED : 1); ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) accs[s][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    int u = 0;
    loadw(0, wc);
    stage_load(0);
#pragma unroll 1
    for (int c = 0; c < A.nch; ++c) {
        __syncthreads();   // the previous chunk's reads are done
        stage_write();
        __syncthreads();
        if (c + 1 < A.nch) stage_load(c + 1);
#pragma unroll 1
        for (int hw = 0; hw < 9; ++hw) {
            const int dh = hw / 3, dw = hw - 3 * dh;
            const unsigned char *lb = smem + ((dh * C3_HW + dw) * C3_HD + m16) * kRowBytes + h4 * 16;
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) {
                ++u;
                loadw(u, wn);   // the next tap's fragments, in flight under this tap's MFMAs
                if constexpr (FULL > 0) {
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        u32x4 bf[NP];
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc)
                            bf[pc] = *reinterpret_cast<const u32x4 *>(
                                lb + pc * C3_PIECE + (((g >> 2) * C3_HW + (g & 3)) * C3_HD + dd) * kRowBytes);
#pragma unroll
                        for (int f = 0; f < FULL; ++f) accf[f][g] = mma_step<T, NP>(wc[f], bf, accf[f][g]);
                    }
                }
                if constexpr (SHARED > 0) {
                    const unsigned char *ls = lb + wave * (C3_HW * C3_HD * kRowBytes);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        u32x4 bf[NP];
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc)
                            bf[pc] = *reinterpret_cast<const u32x4 *>(ls + pc * C3_PIECE + (g * C3_HD + dd) * kRowBytes);
#pragma unroll
                        for (int s = 0; s < SHARED; ++s) accs[s][g] = mma_step<T, NP>(wc[FULL + s], bf, accs[s][g]);
                    }
                }
#pragma unroll
                for (int t = 0; t < NW; ++t)
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc) wc[t][pc] = wn[t][pc];
            }
        }
    }

    // bias, ReLU, store: lane (m16, h4) holds voxel d0 + m16 of its column group, channels 16 tile + 4 h4 + k
    const float *bias = reinterpret_cast<const float *>(A.w + (long long)nunits * NT * NP * kFragBytes);
    float *dst = A.dst + ((long long)b * A.dstC + A.dstOff) * HWD;
    const int d = d0 + m16;
    auto store = [&](int tile, int bh, int bw, f32x4 v) __attribute__((always_inline)) {
        const int h = h0 + bh, w = w0 + bw;
        if (h >= A.H || w >= A.W || d >= A.D) return;
        const long long vox = ((long long)h * A.W + w) * A.D + d;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = 16 * tile + 4 * h4 + k;
            if (o < A.cout) {
                float r = v[k] + bias[o];
                if (A.relu) r = fmaxf(r, 0.0f);
                dst[(long long)o * HWD + vox] = r;
            }
        }
    };
    if constexpr (FULL > 0) {
#pragma unroll
        for (int f = 0; f < FULL; ++f)
#pragma unroll
            for (int g = 0; g < 16; ++g) store(wave + 4 * f, g >> 2, g & 3, accf[f][g]);
    }
    if constexpr (SHARED > 0) {
#pragma unroll
        for (int s = 0; s < SHARED; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) store(4 * FULL + s, wave, g, accs[s][g]);
    }
}

// Packed weights (conv3_pack_elem, mfma_conv.h): fragment ((chunk c, tap t = (kh 3 + kw) 3 + kd), tile), NP pieces of
// [lane][8] 16-bit values each: lane l element j = weight [o = 16 tile + (l & 15)][input channel 32 c + 8 (l >> 4) + j][t],
// zero where o >= cout or the channel >= cin; then 16 nt float32 biases (zero past cout).
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_conv3_pack(const float *__restrict__ w, const float *__restrict__ bias,
                                                    unsigned char *__restrict__ out, int cin, int cout, int nch, int nt) {
    conv3_pack_elem<T, NP>(blockIdx.x * 256 + threadIdx.x, out, cin, cout, nch, nt,
                           [&](int o, int kp, int t) { return w[((long long)o * cin + kp) * 27 + t]; },
                           [&](int o) { return bias[o]; });
}

size_t conv3_packed_bytes(int cin, int cout, int dtype) {
    const int nt = conv3_tiles(cout), nch = (cin + 31) / 32;
    return (size_t)nch * 27 * nt * pieces_of(dtype) * kFragBytes + (size_t)16 * nt * sizeof(float);
}

hipError_t launch_conv3_pack(const float *w, const float *bias, void *packed, int cin, int cout, int dtype,
                             hipStream_t s) {
    const int nt = conv3_tiles(cout), nch = (cin + 31) / 32;
    const unsigned blocks = (unsigned)(nch * 27 * nt * 512 / 256);
    unsigned char *out = static_cast<unsigned char *>(packed);
    with_precision(dtype, [&](auto t, auto np) {
        k_conv3_pack<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(w, bias, out, cin, cout, nch, nt);
    });
    return hipGetLastError();
}

template <int FULL, int SHARED>
static void conv3_launch(const Conv3Args &A, unsigned grid, int dtype, hipStream_t s) {
    with_precision(dtype, [&](auto t, auto np) {
        k_conv3_mfma<decltype(t), decltype(np)::value, FULL, SHARED><<<grid, 256, 0, s>>>(A);
    });
}

// host entry: arguments validated by dvc_conv3 (capi.hip)
hipError_t launch_conv3(const float *src0, int c0, const float *src1, int c1, const void *packed, float *dst,
                        int dst_channels, int dst_offset, int cout, int relu, int B, int H, int W, int D, int dtype,
                        hipStream_t s) {
    Conv3Args A;
    A.s0 = src0; A.s1 = src1 ? src1 : src0; A.w = static_cast<const unsigned char *>(packed); A.dst = dst;
    A.HWD = (long long)H * W * D;
    A.B = B; A.C0 = c0; A.C1 = src1 ? c1 : 0; A.H = H; A.W = W; A.D = D;
    A.dstC = dst_channels; A.dstOff = dst_offset; A.cout = cout; A.relu = relu;
    A.nch = (A.C0 + A.C1 + 31) / 32;
    A.nth = (H + C3_TH - 1) / C3_TH; A.ntw = (W + C3_TW - 1) / C3_TW; A.ntd = (D + C3_TD - 1) / C3_TD;
    const unsigned grid = (unsigned)((long long)B * A.nth * A.ntw * A.ntd);
    switch (conv3_tiles(cout)) {
    case 1: conv3_launch<0, 1>(A, grid, dtype, s); break;
    case 2: conv3_launch<0, 2>(A, grid, dtype, s); break;
    case 4: conv3_launch<1, 0>(A, grid, dtype, s); break;
    case 5: conv3_launch<1, 1>(A, grid, dtype, s); break;
    default: conv3_launch<2, 0>(A, grid, dtype, s); break;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// encoder.convf1: 3 -> 64, 7 x 7 x 7, padding 3, + bias + ReLU
// ---------------------------------------------------------------------------------------------------------------
constexpr int C7_TH = DVC_CONV7_TH, C7_TW = DVC_CONV7_TW, C7_TD = DVC_CONV7_TD;
constexpr int C7_HH = C7_TH + 6, C7_HW = C7_TW + 6, C7_HD = C7_TD + 8;   // D pitch: 22 halo values + 2 zeros
constexpr int C7_CH = C7_HH * C7_HW * C7_HD;
constexpr int C7_COUT = DVC_CONV7_COUT, C7_STEPS = 49;
static_assert(C7_TH == 4 && C7_TW == 4 && C7_TD == 16 && C7_COUT == 64, "four column groups and four tiles per wave");

struct Conv7Args {
    const float *flow;
    const unsigned char *w;   // packed weights (k_conv7_pack), then 64 fp32 biases
    float *dst;
    long long HWD;
    int B, H, W, D, nth, ntw, ntd;
};

template <typename T, int NP>
__global__ __launch_bounds__(256, 1) void k_conv7_flow(Conv7Args A) {
    __shared__ float tile[3 * C7_CH];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b, h0, w0, d0;
    box_of_block(blockIdx.x, A.nth, A.ntw, A.ntd, C7_TH, C7_TW, C7_TD, b, h0, w0, d0);
    const long long HWD = A.HWD;
    const float *src = A.flow + (long long)b * 3 * HWD;

    for (int i = tid; i < 3 * C7_CH; i += 256) {
        const int ci = i / C7_CH, r = i - ci * C7_CH;
        const int hh = r / (C7_HW * C7_HD), rem = r - hh * (C7_HW * C7_HD), ww = rem / C7_HD, dd = rem - ww * C7_HD;
        const int h = h0 - 3 + hh, w = w0 - 3 + ww, d = d0 - 3 + dd;
        const bool ok = dd < C7_TD + 6 && h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
        tile[i] = ok ? src[(long long)ci * HWD + ((long long)h * A.W + w) * A.D + d] : 0.0f;
    }
    __syncthreads();

    const unsigned char *wbase = A.w + lane * 16;
    u32x4 wc[4][NP], wn[4][NP];
    f32x4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane group h4 = input channel (the fourth group is zeros), element j = kd
    const float *lb = tile + (h4 < 3 ? h4 : 0) * C7_CH + wave * (C7_HW * C7_HD) + m16;
    load_frags(wbase, 0, C7_STEPS, 4, wc);
#pragma unroll 1
    for (int u = 0; u < C7_STEPS; ++u) {
        const int kh = u / 7, kw = u - 7 * kh;
        load_frags(wbase, u + 1, C7_STEPS, 4, wn);
        const float *lp = lb + (kh * C7_HW + kw) * C7_HD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 7; ++j) f[j] = h4 < 3 ? lp[g * C7_HD + j] : 0.0f;
            f[7] = 0.0f;
            unsigned hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) split2<T, NP>(f[2 * j], f[2 * j + 1], hi[j], lo[j]);
            u32x4 bf[NP];
            bf[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
            if constexpr (NP == 2) bf[1] = u32x4{lo[0], lo[1], lo[2], lo[3]};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t][g] = mma_step<T, NP>(wc[t], bf, acc[t][g]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) wc[t][pc] = wn[t][pc];
    }

    const float *bias = reinterpret_cast<const float *>(A.w + (long long)C7_STEPS * 4 * NP * kFragBytes);
    float *dst = A.dst + (long long)b * C7_COUT * HWD;
    const int h = h0 + wave, d = d0 + m16;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int w = w0 + g;
        if (h >= A.H || w >= A.W || d >= A.D) continue;
        const long long vox = ((long long)h * A.W + w) * A.D + d;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int o = 16 * t + 4 * h4 + k;
                dst[(long long)o * HWD + vox] = fmaxf(acc[t][g][k] + bias[o], 0.0f);
            }
    }
}

// Packed weights of convf1: fragment (step u = kh 7 + kw, tile), NP pieces of [lane][8]: lane l element j = weight
// [o = 16 tile + (l & 15)][ci = l >> 4][kh][kw][kd = j], zero for ci = 3 or kd = 7; then the 64 biases.
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_conv7_pack(const float *__restrict__ w, const float *__restrict__ bias,
                                                    unsigned char *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C7_STEPS * 4 * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int tile = fr & 3, u = fr >> 2, kh = u / 7, kw = u - 7 * kh;
    const int o = 16 * tile + (l & 15), ci = l >> 4;
    const float v = ci < 3 && j < 7 ? w[((long long)(o * 3 + ci) * 7 + kh) * 49 + kw * 7 + j] : 0.0f;
    pack_store<T, NP>(out, fr, l, j, v);
    if (e < C7_COUT) reinterpret_cast<float *>(out + (long long)C7_STEPS * 4 * NP * kFragBytes)[e] = bias[e];
}

size_t conv7_packed_bytes(int dtype) {
    return (size_t)C7_STEPS * 4 * pieces_of(dtype) * kFragBytes + C7_COUT * sizeof(float);
}

hipError_t launch_conv7_pack(const float *w, const float *bias, void *packed, int dtype, hipStream_t s) {
    const unsigned blocks = C7_STEPS * 4 * 512 / 256;
    unsigned char *out = static_cast<unsigned char *>(packed);
    with_precision(dtype, [&](auto t, auto np) {
        k_conv7_pack<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(w, bias, out);
    });
    return hipGetLastError();
}

// host entry: arguments validated by dvc_conv7_flow (capi.hip)
hipError_t launch_conv7_flow(const float *flow, const void *packed, float *dst, int B, int H, int W, int D, int dtype,
                             hipStream_t s) {
    Conv7Args A;
    A.flow = flow; A.w = static_cast<const unsigned char *>(packed); A.dst = dst;
    A.HWD = (long long)H * W * D;
    A.B = B; A.H = H; A.W = W; A.D = D;
    A.nth = (H + C7_TH - 1) / C7_TH; A.ntw = (W + C7_TW - 1) / C7_TW; A.ntd = (D + C7_TD - 1) / C7_TD;
    const unsigned grid = (unsigned)((long long)B * A.nth * A.ntw * A.ntd);
    with_precision(dtype, [&](auto t, auto np) {
        k_conv7_flow<decltype(t), decltype(np)::value><<<grid, 256, 0, s>>>(A);
    });
    return hipGetLastError();
}

}  // namespace dvc
