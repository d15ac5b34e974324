// encoder.hip -- the feature and context encoders' forward on the matrix cores
// (reference: BottleneckBlock3D, BasicEncoder / MediumEncoder / ShallowEncoder / LateStrideEncoder / FullResEncoder and
// ContextEncoder, src/core/extractor.py:79-301, for input_dim = 1 and norms 'instance' and 'none').
//
// A convolution's raw output (+ bias) is stored once, in float32.  Its InstanceNorm3d and ReLU are applied by whoever
// reads it, as relu(x a[b, c] + s[b, c]) on load; no pass exists only to normalise.  The statistics behind (a, s) are
// per-workgroup sums of x and x^2 in double, written by the producing kernel's epilogue and reduced in a fixed order
// by k_enc_stats: no atomics, so two runs are bit-identical, and no float32 E[x^2] - E[x]^2.
//
//   k_enc_stem      7 x 7 x 7, 1 -> 32 channels, stride 1 or 2, zero padding 3, + bias.  K = 343 taps padded to 352:
//                   eleven steps of v_mfma_f32_16x16x32, k = (kh 7 + kw) 7 + kd.  The single-channel halo box of the
//                   workgroup sits in LDS in float32; a lane builds its eight-value run from dword reads through a
//                   tap -> offset table.
//   k_enc_conv      TAPS = 27 (3 x 3 x 3, padding 1) or 1 (1 x 1 x 1), stride 1 or 2, cin a multiple of 8.  The
//                   prologue (identity, ReLU, or relu(x a + s)) is applied while the input box is staged to LDS as
//                   16-bit rows; out-of-volume voxels are staged as zeros AFTER the prologue's place, so a padding
//                   tap contributes 0 and not relu(s).  K packs taps x channels contiguously:
//                     TAPS = 27  a chunk is 8 input channels, its 27 (tap, 8 channels) units padded to 28 = 7 K-steps
//                                (216 -> 224: 3.6 % zeros; the conv3 packing's 32-channel chunks would spend 75 % of
//                                the matrix work on zeros at cin = 8);
//                     TAPS = 1   a chunk is 32 input channels = one K-step.
//                   Epilogue: bias, then the raw store, or (the context encoder's conv2) tanh on channels
//                   [0, split) and ReLU on the rest, written to two tensors; statistics partials where a norm follows.
//   k_enc_stats     partials -> (scale, shift) = (1 / sqrt(var + eps), -mean scale) per (b, c), biased variance.
//   k_enc_residual  relu(c3 a3 + s3 + shortcut): the only place a block output is materialised.  The shortcut is the
//                   block input (materialised), norm4 of the raw shortcut convolution, or relu(norm1) of the raw stem.
//
// A workgroup (four waves) owns 4 x NG x 16 output voxels along (H, W, D): wave w the NG column groups of 16 voxels
// at h = h0 + w.  NG = 4, but 2 for the strided 3 x 3 x 3 layers, whose 9 x 9 x 33 halo box would not fit 64 KB of
// LDS as float32 rows.  One workgroup computes NTW <= 4 output tiles of 16 channels; wider layers use blockIdx.y.
// Precisions: T = bf16 / fp16, NP = 1: operands rounded once, fp32 accumulation, as conv3.hip.  fp32 is T = bf16 with
// NP = 3 pieces here, not conv3.hip's two: an operand is hi + mid + lo (24 mantissa bits, the float32 value itself)
// and a step takes the six products whose pieces' ranks sum to 2 or less, smallest first.  Two pieces leave a 2^-17
// operand error per layer, which the twenty instance-normalised layers of an encoder compound to 1e-4 of the output
// (measured); three leave the float32 accumulation as the only error.  With NP = 3 the staged box is
// kept in LDS as float32 rows and a lane splits its eight values when it reads them (three 16-bit copies of the
// strided 3 x 3 x 3 halo box would not fit).  Activations between kernels, statistics and outputs are float32 in
// every precision.
#include "enc_common.h"

namespace dvc {

static_assert(EN_TH == 4 && EN_TD == 16, "one wave per output plane of the box, column groups of 16 voxels along D");

long long enc_workgroups(int taps, int stride, int OH, int OW, int OD) {
    const int tw = enc_tw(taps, stride);
    return (long long)((OH + EN_TH - 1) / EN_TH) * ((OW + tw - 1) / tw) * ((OD + EN_TD - 1) / EN_TD);
}

// what the epilogue needs: the output tensor(s) and the statistics partials
struct EncOut {
    const float *bias;   // 16 x packed tiles
    float *y, *y2;       // raw: y (B, cout, ..); split >= 0: y (B, split, ..) tanh, y2 (B, cout - split, ..) ReLU
    double *part;        // [B][nwg][cout][2] sums of x and x^2, or null
    long long OHWD;
    int OH, OW, OD, cout, split, nwg;
};

// acc[t][g]: tile tile0 + t, column group g: lane (m16, h4) holds voxel (h0 + wave, w0 + g, d0 + m16), channels
// 16 (tile0 + t) + 4 h4 + k.  red: LDS, 4 x NTW x 16 x 2 doubles.  Every thread of the workgroup must call it.
template <int NTW, int NG>
__device__ __forceinline__ void enc_epilogue(const EncOut &E, f32x4 (&acc)[NTW][NG], int b, int wg, int tile0, int h0,
                                             int w0, int d0, int wave, int lane, double *red) {
    const int m16 = lane & 15, h4 = lane >> 4;
    const int h = h0 + wave, d = d0 + m16;
    bool ok[NG];
    long long vox[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ok[g] = h < E.OH && w0 + g < E.OW && d < E.OD;
        vox[g] = ((long long)h * E.OW + (w0 + g)) * E.OD + d;
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = 16 * (tile0 + t) + 4 * h4 + k;
            const bool oo = o < E.cout;
            const float bo = E.bias[16 * (tile0 + t) + 4 * h4 + k];
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float v = acc[t][g][k] + bo;
                if (ok[g] && oo) {
                    if (E.split < 0) E.y[((long long)b * E.cout + o) * E.OHWD + vox[g]] = v;
                    else if (o < E.split) E.y[((long long)b * E.split + o) * E.OHWD + vox[g]] = tanhf(v);
                    else E.y2[((long long)b * (E.cout - E.split) + (o - E.split)) * E.OHWD + vox[g]] = fmaxf(v, 0.0f);
                    s += (double)v;
                    q += (double)v * (double)v;
                }
            }
            if (E.part) {   // uniform
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    s += __shfl_xor(s, off);
                    q += __shfl_xor(q, off);
                }
                if (m16 == 0) {
                    double *r = red + ((wave * NTW + t) * 16 + 4 * h4 + k) * 2;
                    r[0] = s;
                    r[1] = q;
                }
            }
        }
    if (E.part) {
        __syncthreads();
        const int tid = wave * 64 + lane;
        if (tid < NTW * 16) {
            const int o = 16 * tile0 + tid;
            if (o < E.cout) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    s += red[((w * NTW) * 16 + tid) * 2];
                    q += red[((w * NTW) * 16 + tid) * 2 + 1];
                }
                double *p = E.part + (((long long)b * E.nwg + wg) * E.cout + o) * 2;
                p[0] = s;
                p[1] = q;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the stem: conv1, 1 -> 32, 7 x 7 x 7
// ---------------------------------------------------------------------------------------------------------------
constexpr int ST_COUT = DVC_ENC_STEM_COUT, ST_K = 343, ST_STEPS = 11;
static_assert(ST_COUT == 32, "two output tiles");

struct EncStemArgs {
    const float *x;
    const unsigned char *w;   // packed weights (k_enc_stem_pack), then 32 fp32 biases
    EncOut E;
    int B, H, W, D, nth, ntw, ntd;
};

template <typename T, int NP, int STRIDE>
__global__ __launch_bounds__(256) void k_enc_stem(EncStemArgs A) {
    constexpr int TW = DVC_ENC_TW;
    constexpr int IH = (EN_TH - 1) * STRIDE + 7, IW = (TW - 1) * STRIDE + 7, ID = (EN_TD - 1) * STRIDE + 7;
    __shared__ float tile[IH * IW * ID];
    __shared__ __attribute__((aligned(16))) int koff[ST_STEPS * 32];
    __shared__ double red[4 * 2 * 16 * 2];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b, h0, w0, d0;
    box_of_block(blockIdx.x, A.nth, A.ntw, A.ntd, EN_TH, TW, EN_TD, b, h0, w0, d0);
    const float *src = A.x + (long long)b * A.H * A.W * A.D;

    for (int i = tid; i < IH * IW * ID; i += 256) {
        const int hh = i / (IW * ID), rem = i - hh * (IW * ID), ww = rem / ID, dd = rem - ww * ID;
        const int h = h0 * STRIDE - 3 + hh, w = w0 * STRIDE - 3 + ww, d = d0 * STRIDE - 3 + dd;
        const bool ok = h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
        tile[i] = ok ? src[((long long)h * A.W + w) * A.D + d] : 0.0f;
    }
    for (int k = tid; k < ST_STEPS * 32; k += 256) {
        const int kh = k / 49, kw = (k - 49 * kh) / 7, kd = k - 49 * kh - 7 * kw;
        koff[k] = k < ST_K ? (kh * IW + kw) * ID + kd : 0;   // padding taps meet zero weights
    }
    __syncthreads();

    const unsigned char *wbase = A.w + lane * 16;
    u32x4 wc[2][NP], wn[2][NP];
    f32x4 acc[2][TW];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < TW; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float *lb = tile + (wave * STRIDE * IW) * ID + m16 * STRIDE;
    load_frags(wbase, 0, ST_STEPS, 2, wc);
#pragma unroll 1
    for (int s = 0; s < ST_STEPS; ++s) {
        load_frags(wbase, s + 1, ST_STEPS, 2, wn);
        int off[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) off[j] = koff[32 * s + 8 * h4 + j];
#pragma unroll
        for (int g = 0; g < TW; ++g) {
            const float *lp = lb + g * STRIDE * ID;
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = lp[off[j]];
            u32x4 bf[NP];
            enc_split8<T, NP>(f, bf);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t][g] = enc_mma<T, NP>(wc[t], bf, acc[t][g]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) wc[t][pc] = wn[t][pc];
    }
    const int wg = (int)(blockIdx.x % (unsigned)A.E.nwg);
    enc_epilogue<2, TW>(A.E, acc, b, wg, 0, h0, w0, d0, wave, lane, red);
}

// Packed weights of the stem: fragment (step s, tile), NP pieces of [lane][8]: lane l element j = weight
// [o = 16 tile + (l & 15)][k = 32 s + 8 (l >> 4) + j], k = (kh 7 + kw) 7 + kd, zero for k >= 343; then the 32 biases.
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_enc_stem_pack(const float *__restrict__ w, const float *__restrict__ bias,
                                                       unsigned char *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ST_STEPS * 2 * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int tile = fr & 1, s = fr >> 1, k = 32 * s + 8 * (l >> 4) + j, o = 16 * tile + (l & 15);
    enc_pack_store<T, NP>(out, fr, l, j, k < ST_K ? w[o * ST_K + k] : 0.0f);
    if (e < ST_COUT) reinterpret_cast<float *>(out + (long long)ST_STEPS * 2 * NP * kFragBytes)[e] = bias[e];
}

size_t enc_stem_packed_bytes(int dtype) {
    return (size_t)ST_STEPS * 2 * enc_pieces(dtype) * kFragBytes + ST_COUT * sizeof(float);
}

hipError_t launch_enc_stem_pack(const float *w, const float *bias, void *packed, int dtype, hipStream_t s) {
    unsigned char *out = static_cast<unsigned char *>(packed);
    enc_with_precision(dtype, [&](auto t, auto np) {
        k_enc_stem_pack<decltype(t), decltype(np)::value><<<ST_STEPS * 2 * 512 / 256, 256, 0, s>>>(w, bias, out);
    });
    return hipGetLastError();
}

static void fill_out(EncOut &E, const unsigned char *packed, size_t frag_bytes, float *y, float *y2, int split,
                     void *partials, int cout, int OH, int OW, int OD, long long nwg) {
    E.bias = reinterpret_cast<const float *>(packed + frag_bytes);
    E.y = y; E.y2 = y2; E.part = static_cast<double *>(partials);
    E.OHWD = (long long)OH * OW * OD;
    E.OH = OH; E.OW = OW; E.OD = OD; E.cout = cout; E.split = split; E.nwg = (int)nwg;
}

// host entry: arguments validated by dvc_enc_stem (capi.hip)
hipError_t launch_enc_stem(const float *x, const void *packed, float *y, void *partials, int B, int H, int W, int D,
                           int stride, int dtype, hipStream_t s) {
    EncStemArgs A;
    A.x = x; A.w = static_cast<const unsigned char *>(packed);
    A.B = B; A.H = H; A.W = W; A.D = D;
    const int OH = enc_out_extent(H, stride), OW = enc_out_extent(W, stride), OD = enc_out_extent(D, stride);
    A.nth = (OH + EN_TH - 1) / EN_TH; A.ntw = (OW + DVC_ENC_TW - 1) / DVC_ENC_TW; A.ntd = (OD + EN_TD - 1) / EN_TD;
    const long long nwg = (long long)A.nth * A.ntw * A.ntd;
    fill_out(A.E, A.w, (size_t)ST_STEPS * 2 * enc_pieces(dtype) * kFragBytes, y, nullptr, -1, partials, ST_COUT, OH, OW,
             OD, nwg);
    const unsigned grid = (unsigned)(B * nwg);
    enc_with_precision(dtype, [&](auto t, auto np) {
        if (stride == 2) k_enc_stem<decltype(t), decltype(np)::value, 2><<<grid, 256, 0, s>>>(A);
        else k_enc_stem<decltype(t), decltype(np)::value, 1><<<grid, 256, 0, s>>>(A);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// the bottleneck's convolutions, the strided shortcut and conv2
// ---------------------------------------------------------------------------------------------------------------
struct EncConvArgs {
    const float *x;
    const float *ss;          // (B, cin, 2) scale and shift of the prologue, or null (scale 1, shift 0)
    const unsigned char *w;   // packed weights (k_enc_conv_pack), then 16 x ntp fp32 biases
    EncOut E;
    long long HWD;
    int B, cin, H, W, D, prologue, nch, ntp, nth, ntw, ntd;
    int SW, SD;               // ZI: the W and D extents of the stored source
};

// ZI (the input gradient of a strided layer, launch_enc_dgrad): the source is read as if zeros stood between its
// voxels: virtual voxel (h, w, d) of the (H, W, D) volume is x[h / 2, w / 2, d / 2] where all three are even, else 0
template <typename T, int NP, int TAPS, int STRIDE, int NTW, bool ZI = false>
__global__ __launch_bounds__(256) void k_enc_conv(EncConvArgs A) {
    static_assert(!ZI || STRIDE == 1, "the zero-inserted source is read at stride 1");
    constexpr int KS = TAPS == 27 ? 3 : 1, NG = enc_tw(TAPS, STRIDE);
    // staged rows: the halo box (TAPS = 27) or just the sampled voxels (TAPS = 1, RSTEP input voxels apart)
    constexpr int RH = TAPS == 27 ? (EN_TH - 1) * STRIDE + 3 : EN_TH, RW = TAPS == 27 ? (NG - 1) * STRIDE + 3 : NG,
                  RD = TAPS == 27 ? (EN_TD - 1) * STRIDE + 3 : EN_TD;
    constexpr int RSTEP = TAPS == 27 ? 1 : STRIDE, OSTEP = TAPS == 27 ? STRIDE : 1;
    constexpr int ROWS = RH * RW * RD;
    constexpr int CPC = TAPS == 27 ? 8 : 32;              // channels per chunk
    constexpr bool F32ROWS = NP == 3;                     // float32 rows, split when read (one LDS copy)
    constexpr int ROWB = F32ROWS ? (TAPS == 27 ? 32 : 144) : (TAPS == 27 ? 16 : kRowBytes);   // LDS row pitch
    constexpr int PIECE = ROWS * ROWB, NPL = F32ROWS ? 1 : NP;
    constexpr int KSTEPS = TAPS == 27 ? 7 : 1;
    constexpr int NST = (ROWS + 255) / 256;               // rows per thread
    static_assert(NPL * PIECE <= 64 * 1024 && NPL * PIECE >= 4 * NTW * 16 * 2 * 8,
                  "the staged box fits LDS and holds the epilogue's reduction scratch after the last chunk");
    __shared__ __attribute__((aligned(16))) unsigned char smem[NPL * PIECE];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b, h0, w0, d0;
    box_of_block(blockIdx.x, A.nth, A.ntw, A.ntd, EN_TH, NG, EN_TD, b, h0, w0, d0);
    const int tile0 = blockIdx.y * NTW;
    const long long HWD = A.HWD;
    const float *src = A.x + (long long)b * A.cin * HWD;
    const float *ss = A.ss ? A.ss + (long long)b * A.cin * 2 : nullptr;

    bool sok[NST];
    long long soff[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int r = tid + 256 * i;
        const int hh = r / (RW * RD), rem = r - hh * (RW * RD), ww = rem / RD, dd = rem - ww * RD;
        const int h = h0 * STRIDE - KS / 2 + hh * RSTEP, w = w0 * STRIDE - KS / 2 + ww * RSTEP,
                  d = d0 * STRIDE - KS / 2 + dd * RSTEP;
        sok[i] = r < ROWS && h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
        if constexpr (ZI) {
            sok[i] = sok[i] && ((h | w | d) & 1) == 0;
            soff[i] = sok[i] ? ((long long)(h >> 1) * A.SW + (w >> 1)) * A.SD + (d >> 1) : 0;
        } else {
            soff[i] = sok[i] ? ((long long)h * A.W + w) * A.D + d : 0;
        }
    }

    float st[NST][CPC];
    auto stage_load = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < CPC; ++k) {
            const int ch = CPC * c + k;
            const bool cok = ch < A.cin;
            const float *p = src + (long long)(cok ? ch : 0) * HWD;
            const float a = ss && cok ? ss[2 * ch] : 1.0f, sh = ss && cok ? ss[2 * ch + 1] : 0.0f;
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                float v = 0.0f;
                if (sok[i] && cok) {   // the activated tensor is what is zero-padded
                    v = p[soff[i]];
                    if (A.prologue == 2) v = fmaf(v, a, sh);
                    if (A.prologue != 0) v = fmaxf(v, 0.0f);
                }
                st[i][k] = v;
            }
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int r = tid + 256 * i;
            if (r >= ROWS) continue;
            if constexpr (F32ROWS) {
#pragma unroll
                for (int o = 0; o < CPC / 4; ++o)
                    *reinterpret_cast<f32x4 *>(smem + r * ROWB + o * 16) =
                        f32x4{st[i][4 * o], st[i][4 * o + 1], st[i][4 * o + 2], st[i][4 * o + 3]};
            } else if constexpr (TAPS == 27) {
                unsigned hi[4], lo[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) split2<T, 1>(st[i][2 * j], st[i][2 * j + 1], hi[j], lo[j]);
                *reinterpret_cast<u32x4 *>(smem + r * ROWB) = u32x4{hi[0], hi[1], hi[2], hi[3]};
            } else {
                stage_row<T, 1>(st[i], smem + r * ROWB, PIECE);
            }
        }
    };

    // fragment ((chunk, K-step), tile, piece); this workgroup's tiles tile0 .. tile0 + NTW - 1
    const unsigned char *wbase = A.w + lane * 16 + (long long)tile0 * NP * kFragBytes;
    const int nunits = A.nch * KSTEPS;
    u32x4 wc[NTW][NP], wn[NTW][NP];
    f32x4 acc[NTW][NG];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    int u = 0;
    load_frags(wbase, 0, nunits, A.ntp, wc);
    stage_load(0);
#pragma unroll 1
    for (int c = 0; c < A.nch; ++c) {
        __syncthreads();   // the previous chunk's reads are done
        stage_write();
        __syncthreads();
        if (c + 1 < A.nch) stage_load(c + 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            ++u;
            load_frags(wbase, u, nunits, A.ntp, wn);
            // this lane's unit of the step: a tap (TAPS = 27; the 28th is padding and meets zero weights) or eight
            // channels of the row (TAPS = 1)
            int row0, coff;
            if constexpr (TAPS == 27) {
                const int q = 4 * s + h4, t = q < 27 ? q : 26;
                const int dh = t / 9, dw = (t - 9 * dh) / 3, dd = t - 9 * dh - 3 * dw;
                row0 = ((wave * OSTEP + dh) * RW + dw) * RD + m16 * OSTEP + dd;
                coff = 0;
            } else {
                row0 = (wave * RW) * RD + m16;
                coff = h4 * (F32ROWS ? 32 : 16);
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                u32x4 bf[NP];
                const unsigned char *lp = smem + (row0 + g * OSTEP * RD) * ROWB + coff;
                if constexpr (F32ROWS) {
                    const f32x4 lo4 = *reinterpret_cast<const f32x4 *>(lp), hi4 = *reinterpret_cast<const f32x4 *>(lp + 16);
                    const float f[8] = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
                    enc_split8<T, NP>(f, bf);
                } else {
                    bf[0] = *reinterpret_cast<const u32x4 *>(lp);
                }
#pragma unroll
                for (int t = 0; t < NTW; ++t) acc[t][g] = enc_mma<T, NP>(wc[t], bf, acc[t][g]);
            }
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) wc[t][pc] = wn[t][pc];
        }
    }
    const int wg = (int)(blockIdx.x % (unsigned)A.E.nwg);
    __syncthreads();   // the last chunk's reads are done: the box's LDS becomes the epilogue's scratch
    enc_epilogue<NTW, NG>(A.E, acc, b, wg, tile0, h0, w0, d0, wave, lane, reinterpret_cast<double *>(smem));
}

// Packed weights of a k_enc_conv layer: fragment ((chunk c, K-step s), tile), NP pieces of [lane][8] 16-bit values:
// lane l element j = weight [o = 16 tile + (l & 15)][ci][tap], where TAPS = 27: tap = 4 s + (l >> 4) (zero for tap 27),
// ci = 8 c + j; TAPS = 1: ci = 32 c + 8 (l >> 4) + j (zero for ci >= cin); zero for o >= cout.  Then 16 ntp biases.
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_enc_conv_pack(const float *__restrict__ w, const float *__restrict__ bias,
                                                       unsigned char *__restrict__ out, int taps, int cin, int cout,
                                                       int nch, int ksteps, int ntp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int nfr = nch * ksteps * ntp;
    if (e >= nfr * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int tile = fr % ntp, cs = fr / ntp, c = cs / ksteps, s = cs - c * ksteps;
    const int o = 16 * tile + (l & 15);
    const int tap = taps == 27 ? 4 * s + (l >> 4) : 0, ci = taps == 27 ? 8 * c + j : 32 * c + 8 * (l >> 4) + j;
    const bool ok = o < cout && ci < cin && tap < taps;
    enc_pack_store<T, NP>(out, fr, l, j, ok ? w[((long long)o * cin + ci) * taps + tap] : 0.0f);
    if (e < 16 * ntp) reinterpret_cast<float *>(out + (long long)nfr * NP * kFragBytes)[e] = e < cout ? bias[e] : 0.0f;
}

size_t enc_conv_packed_bytes(int taps, int cin, int cout, int dtype) {
    const int ntp = enc_ntp(taps, cout);
    return (size_t)enc_nch(taps, cin) * enc_ksteps(taps) * ntp * enc_pieces(dtype) * kFragBytes +
           (size_t)16 * ntp * sizeof(float);
}

hipError_t launch_enc_conv_pack(const float *w, const float *bias, void *packed, int taps, int cin, int cout, int dtype,
                                hipStream_t s) {
    const int ntp = enc_ntp(taps, cout), nch = enc_nch(taps, cin), ks = enc_ksteps(taps);
    const unsigned blocks = (unsigned)(nch * ks * ntp * 512 / 256);
    unsigned char *out = static_cast<unsigned char *>(packed);
    enc_with_precision(dtype, [&](auto t, auto np) {
        k_enc_conv_pack<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(w, bias, out, taps, cin, cout, nch, ks,
                                                                                  ntp);
    });
    return hipGetLastError();
}

template <int TAPS, int STRIDE, int NTW>
static void enc_conv_launch(const EncConvArgs &A, dim3 grid, int dtype, hipStream_t s) {
    enc_with_precision(dtype, [&](auto t, auto np) {
        k_enc_conv<decltype(t), decltype(np)::value, TAPS, STRIDE, NTW><<<grid, 256, 0, s>>>(A);
    });
}

template <int TAPS, int STRIDE>
static void enc_conv_tiles(const EncConvArgs &A, dim3 grid, int ntw, int dtype, hipStream_t s) {
    if (ntw == 1) enc_conv_launch<TAPS, STRIDE, 1>(A, grid, dtype, s);
    else if (ntw == 2) enc_conv_launch<TAPS, STRIDE, 2>(A, grid, dtype, s);
    else if constexpr (TAPS == 1) enc_conv_launch<TAPS, STRIDE, 4>(A, grid, dtype, s);
}

// host entry: arguments validated by dvc_enc_conv (capi.hip)
hipError_t launch_enc_conv(const float *x, const float *scale_shift, int prologue, const void *packed, float *y,
                           float *y2, int split, void *partials, int taps, int stride, int cin, int cout, int B, int H,
                           int W, int D, int dtype, hipStream_t s) {
    EncConvArgs A;
    A.x = x; A.ss = prologue == 2 ? scale_shift : nullptr; A.w = static_cast<const unsigned char *>(packed);
    A.HWD = (long long)H * W * D;
    A.B = B; A.cin = cin; A.H = H; A.W = W; A.D = D; A.prologue = prologue; A.SW = W; A.SD = D;
    A.nch = enc_nch(taps, cin); A.ntp = enc_ntp(taps, cout);
    const int OH = enc_out_extent(H, stride), OW = enc_out_extent(W, stride), OD = enc_out_extent(D, stride);
    const int tw = enc_tw(taps, stride);
    A.nth = (OH + EN_TH - 1) / EN_TH; A.ntw = (OW + tw - 1) / tw; A.ntd = (OD + EN_TD - 1) / EN_TD;
    const long long nwg = (long long)A.nth * A.ntw * A.ntd;
    fill_out(A.E, A.w, (size_t)A.nch * enc_ksteps(taps) * A.ntp * enc_pieces(dtype) * kFragBytes, y, y2, split, partials,
             cout, OH, OW, OD, nwg);
    const int ntw = enc_ntw(taps, cout);
    const dim3 grid((unsigned)(B * nwg), (unsigned)(A.ntp / ntw));
    if (taps == 27) {
        if (stride == 2) enc_conv_tiles<27, 2>(A, grid, ntw, dtype, s);
        else enc_conv_tiles<27, 1>(A, grid, ntw, dtype, s);
    } else {
        if (stride == 2) enc_conv_tiles<1, 2>(A, grid, ntw, dtype, s);
        else enc_conv_tiles<1, 1>(A, grid, ntw, dtype, s);
    }
    return hipGetLastError();
}

template <int TAPS, bool ZI> static void enc_dgrad_tiles(const EncConvArgs &A, dim3 grid, int ntw, int dtype, hipStream_t s) {
    enc_with_precision(dtype, [&](auto t, auto np) {
        using T = decltype(t);
        constexpr int NP = decltype(np)::value;
        if (ntw == 1) k_enc_conv<T, NP, TAPS, 1, 1, ZI><<<grid, 256, 0, s>>>(A);
        else if (ntw == 2) k_enc_conv<T, NP, TAPS, 1, 2, ZI><<<grid, 256, 0, s>>>(A);
        else if constexpr (TAPS == 1) k_enc_conv<T, NP, TAPS, 1, 4, ZI><<<grid, 256, 0, s>>>(A);
    });
}

// The input gradient of a k_enc_conv layer (cin -> cout channels, input volume (H, W, D)): k_enc_conv at stride 1 on
// g (B, cout, OH, OW, OD) with the transposed, flipped weights of k_enc_conv_pack_dgrad (encoder_grad.hip), zero
// biases, no prologue; for a strided layer through the zero-inserted source.  dx (B, cin, H, W, D).  Arguments
// validated by dvc_enc_dgrad (capi.hip).
hipError_t launch_enc_dgrad(const float *g, const void *packed, float *dx, int taps, int stride, int cin, int cout,
                            int B, int H, int W, int D, int dtype, hipStream_t s) {
    EncConvArgs A;
    const int OH = enc_out_extent(H, stride), OW = enc_out_extent(W, stride), OD = enc_out_extent(D, stride);
    A.x = g; A.ss = nullptr; A.w = static_cast<const unsigned char *>(packed);
    A.HWD = (long long)OH * OW * OD;
    A.B = B; A.cin = cout; A.H = H; A.W = W; A.D = D; A.prologue = DVC_ENC_IDENTITY; A.SW = OW; A.SD = OD;
    A.nch = enc_nch(taps, cout); A.ntp = enc_ntp(taps, cin);
    const int tw = enc_tw(taps, 1);
    A.nth = (H + EN_TH - 1) / EN_TH; A.ntw = (W + tw - 1) / tw; A.ntd = (D + EN_TD - 1) / EN_TD;
    const long long nwg = (long long)A.nth * A.ntw * A.ntd;
    fill_out(A.E, A.w, (size_t)A.nch * enc_ksteps(taps) * A.ntp * enc_pieces(dtype) * kFragBytes, dx, nullptr, -1, nullptr,
             cin, H, W, D, nwg);
    const int ntw = enc_ntw(taps, cin);
    const dim3 grid((unsigned)(B * nwg), (unsigned)(A.ntp / ntw));
    if (taps == 27) {
        if (stride == 2) enc_dgrad_tiles<27, true>(A, grid, ntw, dtype, s);
        else enc_dgrad_tiles<27, false>(A, grid, ntw, dtype, s);
    } else {
        if (stride == 2) enc_dgrad_tiles<1, true>(A, grid, ntw, dtype, s);
        else enc_dgrad_tiles<1, false>(A, grid, ntw, dtype, s);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// statistics and the residual
// ---------------------------------------------------------------------------------------------------------------
// one workgroup per (b, c): thread i sums partials i, i + 256, .. in index order, then a fixed tree
__global__ __launch_bounds__(256) void k_enc_stats(const double *__restrict__ part, float *__restrict__ ss, int C,
                                                   int nwg, double count, double eps) {
    __shared__ double rs[256], rq[256];
    const int tid = threadIdx.x, b = blockIdx.x / C, c = blockIdx.x - b * C;
    double s = 0.0, q = 0.0;
    for (int i = tid; i < nwg; i += 256) {
        const double *p = part + (((long long)b * nwg + i) * C + c) * 2;
        s += p[0];
        q += p[1];
    }
    rs[tid] = s;
    rq[tid] = q;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) {
            rs[tid] += rs[tid + n];
            rq[tid] += rq[tid + n];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean = rs[0] / count;
        double var = rq[0] / count - mean * mean;   // in double: the sums carry 53 bits
        var = var > 0.0 ? var : 0.0;
        const double inv = 1.0 / sqrt(var + eps);
        ss[2 * blockIdx.x] = (float)inv;
        ss[2 * blockIdx.x + 1] = (float)(-mean * inv);
    }
}

hipError_t launch_enc_stats(const void *partials, float *scale_shift, int cout, int B, long long nwg, long long count,
                            float eps, hipStream_t s) {
    k_enc_stats<<<(unsigned)(B * cout), 256, 0, s>>>(static_cast<const double *>(partials), scale_shift, cout, (int)nwg,
                                                    (double)count, (double)eps);
    return hipGetLastError();
}

// out = relu(c3 a3 + s3 + r), r = sc (mode 0), sc a4 + s4 (mode 1) or relu(sc a4 + s4) (mode 2); one (b, c) plane per
// blockIdx.y, N = 4 floats per thread where the planes are 16-byte aligned
template <int N>
__global__ __launch_bounds__(256) void k_enc_residual(const float *__restrict__ c3, const float *__restrict__ ss3,
                                                      const float *__restrict__ sc, const float *__restrict__ ss4,
                                                      int mode, float *__restrict__ out, long long HWD) {
    const long long plane = blockIdx.y;
    const float a3 = ss3 ? ss3[2 * plane] : 1.0f, s3 = ss3 ? ss3[2 * plane + 1] : 0.0f;
    const float a4 = ss4 ? ss4[2 * plane] : 1.0f, s4 = ss4 ? ss4[2 * plane + 1] : 0.0f;
    const float *pc = c3 + plane * HWD, *ps = sc + plane * HWD;
    float *po = out + plane * HWD;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * N; i < HWD; i += (long long)gridDim.x * 256 * N) {
        float v[N], r[N];
        if constexpr (N == 4) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(pc + i), c = *reinterpret_cast<const f32x4 *>(ps + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = a[j]; r[j] = c[j]; }
        } else {
            v[0] = pc[i];
            r[0] = ps[i];
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float x = r[j];
            if (mode != 0) x = fmaf(x, a4, s4);
            if (mode == 2) x = fmaxf(x, 0.0f);
            v[j] = fmaxf(fmaf(v[j], a3, s3) + x, 0.0f);
        }
        if constexpr (N == 4) *reinterpret_cast<f32x4 *>(po + i) = f32x4{v[0], v[1], v[2], v[3]};
        else po[i] = v[0];
    }
}

hipError_t launch_enc_residual(const float *c3, const float *ss3, const float *sc, const float *ss4, int mode,
                               float *out, int planes, long long HWD, hipStream_t s) {
    const bool vec = HWD % 4 == 0;
    const long long per = vec ? 1024 : 256;
    const dim3 grid((unsigned)std::min<long long>((HWD + per - 1) / per, 4096), (unsigned)planes);
    if (vec) k_enc_residual<4><<<grid, 256, 0, s>>>(c3, ss3, sc, ss4, mode, out, HWD);
    else k_enc_residual<1><<<grid, 256, 0, s>>>(c3, ss3, sc, ss4, mode, out, HWD);
    return hipGetLastError();
}

}  // namespace dvc
