// conv3_grad.hip -- the backward of k_conv3_mfma (conv3.hip): what a 3 x 3 x 3 layer of the update block needs to
// train (the autograd formula of dvccorr::conv3_ad, dvccorr/library.py).  With y = conv(cat[x, x2], W) + b (+ ReLU) and
// g = dL/dy (times [y > 0] under ReLU):
//   dx   the same convolution with transposed, flipped weights: k_conv3_pack_dgrad writes the fragments of
//        W'[ci][o][t'] = W[o][ci][26 - t'] in k_conv3_pack's layout and k_conv3_mfma runs it unchanged;
//   db   k_conv3_grad_prep: one streaming pass that masks the gradient and sums it per channel;
//   dW   k_conv3_wgrad: dW[o][ci][t] = sum over (b, v) of g[b, o, v] x[b, ci, v + delta(t)], a GEMM whose K runs over
//        the voxels, on v_mfma_f32_16x16x32 with M = output channels (A operand = g), N = input channels (B = x).
//
// k_conv3_wgrad.  A workgroup (four waves) owns one 16-channel ci tile, NT (1 or 2) 16-channel o tiles and all 27
// taps, over a slab of K-blocks; a K-block is the forward's 4 x 4 x 16 voxel box with its 6 x 6 x 18 halo.
//   stage    both operands have K along D, the contiguous axis of both tensors.  Per K-block, g goes to LDS as
//            [o][256 voxels] rows and x as [ci][36 (h, w) halo rows][18 + 6 values] of 16-bit values, D contiguous;
//            out-of-volume voxels and padding channels are zeros.  The row pitches are 16 bytes past a multiple of
//            256, so the 16 channels of a b128 read start on distinct 16-byte slots.  The next K-block's global loads
//            are in flight under the current block's MFMAs.
//   MFMA     one K = 32 step is two columns adjacent along W x 16 d: lane group h4 holds column h4 >> 1, d values
//            8 (h4 & 1) .. + 7.  The A operand is one ds_read_b128.  The B operand of tap (dh, dw, dd) starts dd
//            values off a 16-byte boundary: two aligned b128 reads per (dh, dw) give the ten values the three dd
//            need, and dd = 1 is built with v_alignbyte (dd = 0, 2 are whole dwords).  One set of x rows serves all
//            27 taps; three pre-shifted copies would triple the x image (fp32: 87 KB).
//   split    the waves deal K, not tiles: wave w owns the box's row bh = w (two K steps) with all NT x 27
//            accumulators, so every layer width keeps four waves busy and no LDS read is repeated across waves.  The
//            four partial sums meet once per workgroup, through LDS, in wave order.
//   split-K  the grid is (ci tiles x o groups) x slabs; a slab is `per` consecutive K-blocks of the (B, H, W, D) box
//            grid, per = ceil(nbox / min(nbox, ceil(TARGET / (ci tiles x o groups)))), and only the
//            ceil(nbox / per) slabs that hold a box are launched.  A workgroup writes its partial dW to the
//            workspace [slab][cout][cin][27]; k_conv3_wgrad_reduce sums the slabs in index order.
// Precisions as the forward: T = bf16 / fp16, NP = 1: both operands rounded once, fp32 accumulation; fp32 (T = bf16,
// NP = 2): bf16 hi + lo pieces, g_lo x_hi + g_hi x_lo + g_hi x_hi.
//
// No atomics, no allocation or synchronisation on the host; every sum has a fixed order.
#include "mfma_conv.h"

namespace dvc {

constexpr int WG_KH = DVC_CONV3_WGRAD_KH, WG_KW = DVC_CONV3_WGRAD_KW, WG_KD = DVC_CONV3_WGRAD_KD;
static_assert(WG_KH == 4 && WG_KW == 4 && WG_KD == 16, "four waves x two K = 32 steps of two columns x 16 d");
constexpr int WG_GPITCH = WG_KH * WG_KW * WG_KD * 2 + 16;   // a g row: 256 voxels of 16 bits, + 16 bytes
constexpr int WG_XROW = 48;                                 // an x halo row along D: 18 values + 6 of padding
constexpr int WG_XROWS = (WG_KH + 2) * (WG_KW + 2);         // 36 (h, w) halo rows
constexpr int WG_XPITCH = WG_XROWS * WG_XROW + 80;          // 1808 = 7 x 256 + 16
constexpr int WG_XPIECE = 16 * WG_XPITCH;
constexpr int WG_XIT = 4 * (WG_KH + 2);                     // x pairs (d, d + 1) per staging thread
static_assert(WG_GPITCH % 256 == 16 && WG_XPITCH % 256 == 16, "b128 reads of 16 channels: distinct 16-byte slots");

struct WgradArgs {
    const float *s0, *s1, *g;
    float *ws;
    long long HWD;
    int B, C0, C1, cout, H, W, D, nth, ntw, ntd, nbox, per, nslab, nog;
};

// o tiles per workgroup and the o groups of a layer
static int wgrad_nt(int cout) { return cout <= 16 ? 1 : 2; }
static int wgrad_groups(int cout) { return (cout + 16 * wgrad_nt(cout) - 1) / (16 * wgrad_nt(cout)); }

// the slab rule (see the head of this file)
static void wgrad_slabs(int cin, int cout, int B, int H, int W, int D, int &nbox, int &per, int &nslab) {
    const long long nb = (long long)B * ((H + WG_KH - 1) / WG_KH) * ((W + WG_KW - 1) / WG_KW) * ((D + WG_KD - 1) / WG_KD);
    const long long tiles = (long long)((cin + 15) / 16) * wgrad_groups(cout);
    long long want = (DVC_CONV3_WGRAD_TARGET + tiles - 1) / tiles;
    if (want > nb) want = nb;
    nbox = (int)nb;
    per = (int)((nb + want - 1) / want);
    nslab = (int)((nb + per - 1) / per);
}

size_t conv3_wgrad_workspace_bytes(int cin, int cout, int B, int H, int W, int D) {
    int nbox, per, nslab;
    wgrad_slabs(cin, cout, B, H, W, D, nbox, per, nslab);
    return (size_t)nslab * cout * cin * 27 * sizeof(float);
}

template <typename T, int NP, int NT>
__global__ __launch_bounds__(256, 1) void k_conv3_wgrad(WgradArgs A) {
    constexpr int GPIECE = 16 * NT * WG_GPITCH;
    constexpr int GIT = 8 * NT;   // g pairs per thread
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * (GPIECE + WG_XPIECE)];
    static_assert(NP * (GPIECE + WG_XPIECE) >= 4 * 3 * 1024, "the epilogue's exchange buffer");
    unsigned char *gs = smem, *xs = smem + NP * GPIECE;
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = blockIdx.x;
    const int slab = (int)(bid % (unsigned)A.nslab);
    bid /= (unsigned)A.nslab;
    const int og = (int)(bid % (unsigned)A.nog), cit = (int)(bid / (unsigned)A.nog);
    const int cin = A.C0 + A.C1, o0 = 16 * NT * og, c0 = 16 * cit;
    const long long HWD = A.HWD;

    // g staging: this thread's pair (d, d + 1) of column (gbh, gbw), channels o0 + go + 2 i
    const int gq = tid & 127, gbh = gq >> 5, gbw = (gq >> 3) & 3, gd = 2 * (gq & 7), go = tid >> 7;
    // x staging: threads 0..215 own the 6 x 9 (ww, d pair) halo columns of four channel phases
    const int xdp = tid % 9, xww = (tid / 9) % (WG_KW + 2), xcs = tid / (9 * (WG_KW + 2));
    float gv[GIT][2], xv[WG_XIT][2];

    auto stage_load = [&](int bx) __attribute__((always_inline)) {
        int b, h0, w0, d0;
        box_of_block((unsigned)bx, A.nth, A.ntw, A.ntd, WG_KH, WG_KW, WG_KD, b, h0, w0, d0);
        {
            const int h = h0 + gbh, w = w0 + gbw, d = d0 + gd;
            const bool ok0 = h < A.H && w < A.W && d < A.D, ok1 = ok0 && d + 1 < A.D;
            const long long voff = ((long long)h * A.W + w) * A.D + d;
            const float *gb = A.g + (long long)b * A.cout * HWD;
#pragma unroll
            for (int i = 0; i < GIT; ++i) {
                const int o = o0 + go + 2 * i;
                const bool oo = o < A.cout;
                gv[i][0] = ok0 && oo ? gb[(long long)o * HWD + voff] : 0.0f;
                gv[i][1] = ok1 && oo ? gb[(long long)o * HWD + voff + 1] : 0.0f;
            }
        }
        // x: this thread's pair of halo column (ww, dp), rows hh = 0..5, channels c0 + xcs + 4 k
        const float *s0 = A.s0 + (long long)b * A.C0 * HWD;
        const float *s1 = A.s1 + (long long)b * A.C1 * HWD;   // never read when C1 = 0
        const int w = w0 - 1 + xww, d = d0 - 1 + 2 * xdp;
        const bool okw = xcs < 4 && w >= 0 && w < A.W;
        const bool okd0 = okw && d >= 0 && d < A.D, okd1 = okw && d + 1 < A.D;
        const long long xoff = ((long long)(h0 - 1) * A.W + w) * A.D + d, WD = (long long)A.W * A.D;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + xcs + 4 * k;
            const float *p = (c < A.C0 ? s0 + (long long)c * HWD : s1 + (long long)(c - A.C0) * HWD) + xoff;
#pragma unroll
            for (int hh = 0; hh < WG_KH + 2; ++hh) {
                const int h = h0 - 1 + hh;
                const bool okh = c < cin && h >= 0 && h < A.H;
                xv[k * (WG_KH + 2) + hh][0] = okh && okd0 ? p[hh * WD] : 0.0f;
                xv[k * (WG_KH + 2) + hh][1] = okh && okd1 ? p[hh * WD + 1] : 0.0f;
            }
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < GIT; ++i) {
            unsigned hi, lo;
            split2<T, NP>(gv[i][0], gv[i][1], hi, lo);
            unsigned char *p = gs + (go + 2 * i) * WG_GPITCH + gq * 4;
            *reinterpret_cast<unsigned *>(p) = hi;
            if constexpr (NP == 2) *reinterpret_cast<unsigned *>(p + GPIECE) = lo;
        }
        if (xcs < 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int hh = 0; hh < WG_KH + 2; ++hh) {
                    unsigned hi, lo;
                    split2<T, NP>(xv[k * (WG_KH + 2) + hh][0], xv[k * (WG_KH + 2) + hh][1], hi, lo);
                    unsigned char *p = xs + (xcs + 4 * k) * WG_XPITCH + (hh * (WG_KW + 2) + xww) * WG_XROW + xdp * 4;
                    *reinterpret_cast<unsigned *>(p) = hi;
                    if constexpr (NP == 2) *reinterpret_cast<unsigned *>(p + WG_XPIECE) = lo;
                }
        }
    };

    f32x4 acc[NT][27];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[t][k] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane (m16, h4): A = g row of channel m16, B = x rows of channel m16; column h4 >> 1 of the pair, d half h4 & 1
    const unsigned char *ga = gs + m16 * WG_GPITCH + wave * (WG_KW * WG_KD * 2) + h4 * 16;
    const unsigned char *xb = xs + m16 * WG_XPITCH + (wave * (WG_KW + 2) + (h4 >> 1)) * WG_XROW + (h4 & 1) * 16;

    int bx = slab * A.per;
    const int bend = bx + A.per < A.nbox ? bx + A.per : A.nbox;
    stage_load(bx);
#pragma unroll 1
    for (; bx < bend; ++bx) {
        __syncthreads();   // the previous K-block's reads are done
        stage_write();
        __syncthreads();
        if (bx + 1 < bend) stage_load(bx + 1);
#pragma unroll 1
        for (int p = 0; p < 2; ++p) {
            u32x4 af[NT][NP];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
                    af[t][pc] = *reinterpret_cast<const u32x4 *>(ga + pc * GPIECE + t * 16 * WG_GPITCH + p * 64);
#pragma unroll
            for (int hw = 0; hw < 9; ++hw) {
                const int dh = hw / 3, dw = hw - 3 * dh;
                const unsigned char *xp = xb + (dh * (WG_KW + 2) + 2 * p + dw) * WG_XROW;
                u32x4 q0[NP], q1[NP];
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) {
                    q0[pc] = *reinterpret_cast<const u32x4 *>(xp + pc * WG_XPIECE);
                    q1[pc] = *reinterpret_cast<const u32x4 *>(xp + pc * WG_XPIECE + 16);
                }
#pragma unroll
                for (int dd = 0; dd < 3; ++dd) {
                    u32x4 bf[NP];
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc) {
                        const u32x4 a = q0[pc];
                        const unsigned n = q1[pc][0];
                        if (dd == 0) bf[pc] = a;
                        else if (dd == 2) bf[pc] = u32x4{a[1], a[2], a[3], n};
                        else
                            bf[pc] = u32x4{__builtin_amdgcn_alignbyte(a[1], a[0], 2), __builtin_amdgcn_alignbyte(a[2], a[1], 2),
                                           __builtin_amdgcn_alignbyte(a[3], a[2], 2), __builtin_amdgcn_alignbyte(n, a[3], 2)};
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t][hw * 3 + dd] = mma_step<T, NP>(af[t], bf, acc[t][hw * 3 + dd]);
                }
            }
        }
    }

    // the four waves' partial sums meet in LDS, three accumulators per round, summed in wave order.  Lane (m16, h4)
    // holds input channel c0 + m16, output channels o0 + 16 tile + 4 h4 + k.
    float *red = reinterpret_cast<float *>(smem);
    float *wsl = A.ws + (long long)slab * A.cout * cin * 27;
    const int rl = tid >> 2, rk = tid & 3;
    const int rci = c0 + (rl & 15);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ro = o0 + 16 * t + 4 * (rl >> 4) + rk;
#pragma unroll
        for (int hw = 0; hw < 9; ++hw) {
            __syncthreads();   // the main loop's reads, or the previous round's, are done
#pragma unroll
            for (int dd = 0; dd < 3; ++dd)
                *reinterpret_cast<f32x4 *>(red + ((wave * 3 + dd) * 64 + lane) * 4) = acc[t][hw * 3 + dd];
            __syncthreads();
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) {
                const float s = ((red[dd * 256 + tid] + red[768 + dd * 256 + tid]) + red[1536 + dd * 256 + tid]) +
                                red[2304 + dd * 256 + tid];
                if (ro < A.cout && rci < cin) wsl[((long long)ro * cin + rci) * 27 + hw * 3 + dd] = s;
            }
        }
    }
}

// dW[e] = the slabs' partials of element e, summed in slab order
__global__ __launch_bounds__(256) void k_conv3_wgrad_reduce(const float *__restrict__ ws, float *__restrict__ dw, int n,
                                                            int nslab) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = 0.0f;
    for (int k = 0; k < nslab; ++k) s += ws[(long long)k * n + e];
    dw[e] = s;
}

// the split-K reduce on its own: k_gru_wgrad (gru_grad.hip) shares it
hipError_t launch_wgrad_reduce(const float *ws, float *dw, int n, int nslab, hipStream_t s) {
    k_conv3_wgrad_reduce<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(ws, dw, n, nslab);
    return hipGetLastError();
}

// host entry: arguments validated by dvc_conv3_wgrad (capi.hip)
hipError_t launch_conv3_wgrad(const float *src0, int c0, const float *src1, int c1, const float *g, int cout, float *dw,
                              void *workspace, int B, int H, int W, int D, int dtype, hipStream_t s) {
    WgradArgs A;
    A.s0 = src0; A.s1 = src1 ? src1 : src0; A.g = g; A.ws = static_cast<float *>(workspace);
    A.HWD = (long long)H * W * D;
    A.B = B; A.C0 = c0; A.C1 = src1 ? c1 : 0; A.cout = cout; A.H = H; A.W = W; A.D = D;
    A.nth = (H + WG_KH - 1) / WG_KH; A.ntw = (W + WG_KW - 1) / WG_KW; A.ntd = (D + WG_KD - 1) / WG_KD;
    const int cin = A.C0 + A.C1;
    wgrad_slabs(cin, cout, B, H, W, D, A.nbox, A.per, A.nslab);
    A.nog = wgrad_groups(cout);
    const unsigned grid = (unsigned)(A.nslab * A.nog * ((cin + 15) / 16));
    with_precision(dtype, [&](auto t, auto np) {
        if (wgrad_nt(cout) == 1) k_conv3_wgrad<decltype(t), decltype(np)::value, 1><<<grid, 256, 0, s>>>(A);
        else k_conv3_wgrad<decltype(t), decltype(np)::value, 2><<<grid, 256, 0, s>>>(A);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wgrad_reduce(A.ws, dw, cout * cin * 27, A.nslab, s);
}

// ---------------------------------------------------------------------------------------------------------------
// the input gradient's weights: W'[ci][o][t'] = W[o][ci][26 - t'] in k_conv3_pack's layout, zero biases
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_conv3_pack_dgrad(const float *__restrict__ w, unsigned char *__restrict__ out,
                                                          int cin, int cout, int nch, int nt) {
    // a layer with cout input channels (the chunks) and cin output channels (the tiles)
    conv3_pack_elem<T, NP>(blockIdx.x * 256 + threadIdx.x, out, cout, cin, nch, nt,
                           [&](int o, int kp, int t) { return w[((long long)kp * cin + o) * 27 + 26 - t]; },
                           [](int) { return 0.0f; });
}

hipError_t launch_conv3_pack_dgrad(const float *w, void *packed, int cin, int cout, int dtype, hipStream_t s) {
    const int nt = conv3_tiles(cin), nch = (cout + 31) / 32;
    const unsigned blocks = (unsigned)(nch * 27 * nt * 512 / 256);
    unsigned char *out = static_cast<unsigned char *>(packed);
    with_precision(dtype, [&](auto t, auto np) {
        k_conv3_pack_dgrad<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(w, out, cin, cout, nch, nt);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// k_conv3_grad_prep: g = grad_y [y > 0] (RELU) and the bias gradient's partial sums, one streaming pass.  Workgroup
// (chunk, o, b) owns DVC_CONV3_PREP_CHUNK consecutive voxels of channel o of batch element b; a thread sums its
// values in index order, a wave by a shuffle tree, the four waves in wave order: partial[o][b][chunk].
// k_conv3_db_reduce then sums a channel's B x nchunk partials in index order.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PREP_CHUNK = DVC_CONV3_PREP_CHUNK;
static_assert(PREP_CHUNK == 4096, "256 threads x 4 float4");

template <bool RELU, bool VEC>
__global__ __launch_bounds__(256) void k_conv3_grad_prep(const float *__restrict__ gy, const float *__restrict__ y,
                                                         float *__restrict__ g, float *__restrict__ partial,
                                                         long long HWD, int cout, int B, int nchunk) {
    __shared__ float wsum[4];
    const int tid = threadIdx.x, chunk = blockIdx.x, o = blockIdx.y, b = blockIdx.z;
    const long long row = ((long long)b * cout + o) * HWD, start = (long long)chunk * PREP_CHUNK;
    float s = 0.0f;
    if constexpr (VEC) {   // HWD is a multiple of four and the pointers are 16-byte aligned
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long idx = start + (long long)(i * 256 + tid) * 4;
            if (idx < HWD) {
                f32x4 v = *reinterpret_cast<const f32x4 *>(gy + row + idx);
                if constexpr (RELU) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(y + row + idx);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = a[k] > 0.0f ? v[k] : 0.0f;
                    *reinterpret_cast<f32x4 *>(g + row + idx) = v;
                }
                s += (v[0] + v[1]) + (v[2] + v[3]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long idx = start + i * 256 + tid;
            if (idx < HWD) {
                float v = gy[row + idx];
                if constexpr (RELU) {
                    v = y[row + idx] > 0.0f ? v : 0.0f;
                    g[row + idx] = v;
                }
                s += v;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[((long long)o * B + b) * nchunk + chunk] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(128) void k_conv3_db_reduce(const float *__restrict__ partial, float *__restrict__ db,
                                                         int cout, int n) {
    const int o = blockIdx.x * 128 + threadIdx.x;
    if (o >= cout) return;
    float s = 0.0f;
    for (int k = 0; k < n; ++k) s += partial[(long long)o * n + k];
    db[o] = s;
}

// host entry: arguments validated by dvc_conv3_grad_prep (capi.hip); y and g are both set (ReLU) or both null
hipError_t launch_conv3_grad_prep(const float *grad_y, const float *y, float *g, float *db, float *partial, int cout,
                                  int B, int H, int W, int D, hipStream_t s) {
    const long long HWD = (long long)H * W * D;
    const int nchunk = (int)((HWD + PREP_CHUNK - 1) / PREP_CHUNK);
    const dim3 grid((unsigned)nchunk, (unsigned)cout, (unsigned)B);
    const bool vec = HWD % 4 == 0 && ((uintptr_t)grad_y | (uintptr_t)y | (uintptr_t)g) % 16 == 0;
    if (y) {
        if (vec) k_conv3_grad_prep<true, true><<<grid, 256, 0, s>>>(grad_y, y, g, partial, HWD, cout, B, nchunk);
        else k_conv3_grad_prep<true, false><<<grid, 256, 0, s>>>(grad_y, y, g, partial, HWD, cout, B, nchunk);
    } else {
        if (vec) k_conv3_grad_prep<false, true><<<grid, 256, 0, s>>>(grad_y, y, g, partial, HWD, cout, B, nchunk);
        else k_conv3_grad_prep<false, false><<<grid, 256, 0, s>>>(grad_y, y, g, partial, HWD, cout, B, nchunk);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_conv3_db_reduce<<<(unsigned)((cout + 127) / 128), 128, 0, s>>>(partial, db, cout, B * nchunk);
    return hipGetLastError();
}

}  // namespace dvc
