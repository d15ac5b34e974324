// encoder_grad.hip -- the backward of the encoders' forward (encoder.hip): what dvccorr.encoder_ad and
// dvccorr.context_encoder_ad need to train the feature and context encoders (dvccorr/library.py, dvccorr::encoder_ad).
//
// For a raw convolution output x with the table a = 1 / sqrt(var + eps), s = -mean a, n = fma(x, a, s) as the forward's
// prologue evaluates it, and gn the gradient with respect to n after the consumer's mask:
//   k_enc_ng_sums    per-workgroup double partials of sum(gn) and sum(gn n) per (b, c) plane, gn = g [n > 0] (mask 1) or g;
//   k_enc_ng_apply   g_x = a (gn - m1 - n m2), m1 = mean(gn), m2 = mean(gn n): every workgroup of a plane sums the plane's
//                    partials in index order (the same value everywhere), and leaves a double partial of sum(g_x) for the
//                    bias gradient.  Without a table (norm 'none') g_x = gn and k_enc_ng_sums does not run;
//   k_enc_db_reduce  db[c] = the (b, chunk) partials of channel c summed in index order.
//   k_enc_grad_add   dst = (a + b) [m > 0]: the gradient of a block input is conv1's input gradient plus the shortcut
//                    path's, masked by the ReLU that produced the stored block output m; b and m are optional.
//   k_enc_split_grad conv2 of the context encoder: g = g_net (1 - net^2) on channels [0, split), g_ctx [ctx > 0] behind.
//   k_enc_conv_pack_dgrad   W'[ci][o][t'] = W[o][ci][taps - 1 - t'] in k_enc_conv_pack's layout with zero biases:
//                    k_enc_conv runs the input gradient unchanged (launch_enc_dgrad, encoder.hip), a strided layer's
//                    through its zero-inserted source mode.
//   k_enc_wgrad      dW[o][ci][t] = sum over (b, v) of g_x[b, o, v] act(in)[b, ci, v stride + delta(t)]: a split-K GEMM on
//                    v_mfma_f32_16x16x32 whose K runs over the output voxels, for 1 x 1 x 1, 3 x 3 x 3 and the stem's
//                    7 x 7 x 7 (cin = 1), strides 1 and 2.
//
// k_enc_wgrad.  M = output channels (A operand = g_x), N = the layer's taps x cin weight columns, column n = tap cin +
// ci, in tiles of 16: the narrow 3 x 3 x 3 layers (8, 16, 24 channels) fill their N tiles with (tap, channel) pairs
// (216 columns in 14 tiles at cin = 8, 3.6 % padding) instead of running one tap's 8 channels in a tile of 16.  A K step is
// 32 consecutive output voxels of one batch element in memory order; lane group h4 holds voxels 8 h4 .. + 7.  Both
// operands come straight from global memory: g_x is contiguous along K, and a lane's column fixes its (tap, channel),
// so its eight input values are one gather with the bounds test and the forward's prologue (identity, ReLU,
// relu(fma(x, a, s)); out-of-volume taps are zeros of the ACTIVATED tensor) applied per value.  No LDS tile exists
// that would serve all columns of a step: the taps' reuse of the input is left to the caches (see DESIGN.md 4.17 for
// what that costs).  A workgroup owns MT = 2 row tiles x NTN (7, or 2 for 1 x 1 x 1) column tiles; its four waves deal
// the K steps of the slab round-robin and meet once, through LDS, in wave order.  The grid is (row groups x column
// groups) x slabs of `per` consecutive K steps; a slab's partial goes to the workspace [slab][cout][cin][taps] and
// k_conv3_wgrad_reduce sums the slabs in index order.  No atomics: bit-identical from run to run.
// Precisions as the forward: one rounding of both operands (bf16 / fp16), or three bf16 pieces and six products (fp32).
#include "enc_common.h"

namespace dvc {

hipError_t launch_wgrad_reduce(const float *ws, float *dw, int n, int nslab, hipStream_t s);   // conv3_grad.hip

// ---------------------------------------------------------------------------------------------------------------
// the weight gradient
// ---------------------------------------------------------------------------------------------------------------
constexpr int EW_MT = 2;
constexpr int ew_ntn(int ks) { return ks == 1 ? 2 : 7; }

struct EncWgradArgs {
    const float *x, *ss, *g;
    float *ws;
    long long HWD, OHWD;
    int cin, cout, H, W, D, OW, OD, prologue, ncols, ngroups, kpb, nk, per, nslab;
};

struct EncWgradPlan { int ngroups, nmg, kpb, nk, per, nslab; };

static EncWgradPlan enc_wgrad_plan(int taps, int stride, int cin, int cout, int B, int H, int W, int D) {
    const int ks = taps == 1 ? 1 : taps == 27 ? 3 : 7;
    const long long ohwd = (long long)enc_out_extent(H, stride) * enc_out_extent(W, stride) * enc_out_extent(D, stride);
    EncWgradPlan P;
    const int ntiles = (taps * cin + 15) / 16;
    P.ngroups = (ntiles + ew_ntn(ks) - 1) / ew_ntn(ks);
    P.nmg = (cout + 16 * EW_MT - 1) / (16 * EW_MT);
    P.kpb = (int)((ohwd + 31) / 32);
    P.nk = B * P.kpb;
    long long want = (DVC_ENC_WGRAD_TARGET + P.ngroups * P.nmg - 1) / (P.ngroups * P.nmg);
    const long long most = (P.nk + 3) / 4;   // a slab gives each wave a K step
    if (want > most) want = most;
    P.per = (int)((P.nk + want - 1) / want);
    P.nslab = (P.nk + P.per - 1) / P.per;
    return P;
}

size_t enc_wgrad_workspace_bytes(int taps, int stride, int cin, int cout, int B, int H, int W, int D) {
    return (size_t)enc_wgrad_plan(taps, stride, cin, cout, B, H, W, D).nslab * cout * cin * taps * sizeof(float);
}

template <typename T, int NP, int KS, int STRIDE>
__global__ __launch_bounds__(256) void k_enc_wgrad(EncWgradArgs A) {
    constexpr int TAPS = KS * KS * KS, PAD = KS / 2, NTN = ew_ntn(KS), MT = EW_MT;
    __shared__ __attribute__((aligned(16))) float red[4 * 256];
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = blockIdx.x;
    const int slab = (int)(bid % (unsigned)A.nslab);
    bid /= (unsigned)A.nslab;
    const int grp = (int)(bid % (unsigned)A.ngroups), mg = (int)(bid / (unsigned)A.ngroups);

    // this lane's weight column of each tile: input channel, tap offsets
    int cch[NTN], cdh[NTN], cdw[NTN], cdd[NTN];
    bool cok[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t) {
        const int n = (grp * NTN + t) * 16 + m16;
        cok[t] = n < A.ncols;
        const int tap = cok[t] ? n / A.cin : 0;
        cch[t] = cok[t] ? n - tap * A.cin : 0;
        cdh[t] = tap / (KS * KS) - PAD;
        cdw[t] = (tap / KS) % KS - PAD;
        cdd[t] = tap % KS - PAD;
    }
    const int ntile = (A.ncols + 15) / 16 - grp * NTN;   // valid tiles of this group (uniform)

    f32x4 acc[MT][NTN];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTN; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int k0 = slab * A.per, k1 = k0 + A.per < A.nk ? k0 + A.per : A.nk;
    const int OWD = A.OW * A.OD;
#pragma unroll 1
    for (int ks = k0 + wave; ks < k1; ks += 4) {
        const int b = ks / A.kpb;
        const long long vbase = (long long)(ks - b * A.kpb) * 32 + 8 * h4;
        // the lane's eight output voxels: input coordinates of tap (0, 0, 0) - PAD, and whether the voxel exists
        int ih[8], iw[8], id[8];
        unsigned vok = 0;
        {
            int oh = (int)(vbase / OWD);
            const int r = (int)(vbase - (long long)oh * OWD);
            int ow = r / A.OD, od = r - ow * A.OD;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (vbase + j < A.OHWD) vok |= 1u << j;
                ih[j] = oh * STRIDE;
                iw[j] = ow * STRIDE;
                id[j] = od * STRIDE;
                if (++od == A.OD) {
                    od = 0;
                    if (++ow == A.OW) {
                        ow = 0;
                        ++oh;
                    }
                }
            }
        }
        u32x4 af[MT][NP];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int o = (mg * MT + m) * 16 + m16;
            const float *gp = A.g + ((long long)b * A.cout + (o < A.cout ? o : 0)) * A.OHWD + vbase;
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = (o < A.cout && (vok >> j & 1)) ? gp[j] : 0.0f;
            enc_split8<T, NP>(f, af[m]);
        }
#pragma unroll
        for (int t = 0; t < NTN; ++t) {
            if (t >= ntile) break;   // uniform
            const float *xp = A.x + ((long long)b * A.cin + cch[t]) * A.HWD;
            float a = 1.0f, sh = 0.0f;
            if (A.prologue == DVC_ENC_NORM_RELU) {
                a = A.ss[((long long)b * A.cin + cch[t]) * 2];
                sh = A.ss[((long long)b * A.cin + cch[t]) * 2 + 1];
            }
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int h = ih[j] + cdh[t], w = iw[j] + cdw[t], d = id[j] + cdd[t];
                const bool ok = cok[t] && (vok >> j & 1) && h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
                float v = 0.0f;
                if (ok) {   // the activated tensor is what is zero-padded
                    v = xp[((long long)h * A.W + w) * A.D + d];
                    if (A.prologue == DVC_ENC_NORM_RELU) v = fmaf(v, a, sh);
                    if (A.prologue != DVC_ENC_IDENTITY) v = fmaxf(v, 0.0f);
                }
                f[j] = v;
            }
            u32x4 bf[NP];
            enc_split8<T, NP>(f, bf);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m][t] = enc_mma<T, NP>(af[m], bf, acc[m][t]);
        }
    }

    // the four waves' partial sums meet in LDS, one accumulator per round, summed in wave order.  Lane (m16, h4) holds
    // column n = 16 tile + m16 and rows o = 16 (mg MT + m) + 4 h4 + k; thread tid sums value k = tid >> 6 of lane tid & 63.
    float *wsl = A.ws + (long long)slab * A.cout * A.ncols;
    const int rk = tid >> 6;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTN; ++t) {
            if (t >= ntile) break;   // uniform
            __syncthreads();   // the previous round's reads are done
            *reinterpret_cast<f32x4 *>(red + (wave * 64 + lane) * 4) = acc[m][t];
            __syncthreads();
            const float s = ((red[lane * 4 + rk] + red[256 + lane * 4 + rk]) + red[512 + lane * 4 + rk]) +
                            red[768 + lane * 4 + rk];
            const int o = (mg * MT + m) * 16 + 4 * h4 + rk, n = (grp * NTN + t) * 16 + m16;
            if (o < A.cout && n < A.ncols) {
                const int tap = n / A.cin, ci = n - tap * A.cin;
                wsl[((long long)o * A.cin + ci) * TAPS + tap] = s;
            }
        }
}

template <int KS, int STRIDE> static void enc_wgrad_launch(const EncWgradArgs &A, unsigned grid, int dtype, hipStream_t s) {
    enc_with_precision(dtype, [&](auto t, auto np) {
        k_enc_wgrad<decltype(t), decltype(np)::value, KS, STRIDE><<<grid, 256, 0, s>>>(A);
    });
}

// host entry: arguments validated by dvc_enc_wgrad / dvc_enc_stem_wgrad (capi.hip); taps 1, 27 or 343 (cin = 1)
hipError_t launch_enc_wgrad(const float *x, const float *scale_shift, int prologue, const float *g, float *dw,
                            void *workspace, int taps, int stride, int cin, int cout, int B, int H, int W, int D,
                            int dtype, hipStream_t s) {
    EncWgradArgs A;
    const EncWgradPlan P = enc_wgrad_plan(taps, stride, cin, cout, B, H, W, D);
    const int OH = enc_out_extent(H, stride);
    A.x = x; A.ss = scale_shift; A.g = g; A.ws = static_cast<float *>(workspace);
    A.OW = enc_out_extent(W, stride); A.OD = enc_out_extent(D, stride);
    A.HWD = (long long)H * W * D; A.OHWD = (long long)OH * A.OW * A.OD;
    A.cin = cin; A.cout = cout; A.H = H; A.W = W; A.D = D; A.prologue = prologue; A.ncols = taps * cin;
    A.ngroups = P.ngroups; A.kpb = P.kpb; A.nk = P.nk; A.per = P.per; A.nslab = P.nslab;
    const unsigned grid = (unsigned)(P.nslab * P.ngroups * P.nmg);
    if (taps == 1) {
        if (stride == 2) enc_wgrad_launch<1, 2>(A, grid, dtype, s);
        else enc_wgrad_launch<1, 1>(A, grid, dtype, s);
    } else if (taps == 27) {
        if (stride == 2) enc_wgrad_launch<3, 2>(A, grid, dtype, s);
        else enc_wgrad_launch<3, 1>(A, grid, dtype, s);
    } else {
        if (stride == 2) enc_wgrad_launch<7, 2>(A, grid, dtype, s);
        else enc_wgrad_launch<7, 1>(A, grid, dtype, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wgrad_reduce(A.ws, dw, cout * cin * taps, P.nslab, s);
}

// ---------------------------------------------------------------------------------------------------------------
// the input gradient's weights
// ---------------------------------------------------------------------------------------------------------------
// k_enc_conv_pack's fragments of the layer with cout input channels (the chunks) and cin output channels (the tiles)
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_enc_conv_pack_dgrad(const float *__restrict__ w, unsigned char *__restrict__ out,
                                                             int taps, int cin, int cout, int nch, int ksteps, int ntp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int nfr = nch * ksteps * ntp;
    if (e >= nfr * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int tile = fr % ntp, cs = fr / ntp, c = cs / ksteps, s = cs - c * ksteps;
    const int ci = 16 * tile + (l & 15);   // the gradient's output channel
    const int tap = taps == 27 ? 4 * s + (l >> 4) : 0, o = taps == 27 ? 8 * c + j : 32 * c + 8 * (l >> 4) + j;
    const bool ok = ci < cin && o < cout && tap < taps;
    enc_pack_store<T, NP>(out, fr, l, j, ok ? w[((long long)o * cin + ci) * taps + (taps - 1 - tap)] : 0.0f);
    if (e < 16 * ntp) reinterpret_cast<float *>(out + (long long)nfr * NP * kFragBytes)[e] = 0.0f;
}

size_t enc_dgrad_packed_bytes(int taps, int cin, int cout, int dtype) {
    const int ntp = enc_ntp(taps, cin);
    return (size_t)enc_nch(taps, cout) * enc_ksteps(taps) * ntp * enc_pieces(dtype) * kFragBytes +
           (size_t)16 * ntp * sizeof(float);
}

hipError_t launch_enc_conv_pack_dgrad(const float *w, void *packed, int taps, int cin, int cout, int dtype,
                                      hipStream_t s) {
    const int ntp = enc_ntp(taps, cin), nch = enc_nch(taps, cout), ks = enc_ksteps(taps);
    const unsigned blocks = (unsigned)(nch * ks * ntp * 512 / 256);
    unsigned char *out = static_cast<unsigned char *>(packed);
    enc_with_precision(dtype, [&](auto t, auto np) {
        k_enc_conv_pack_dgrad<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(w, out, taps, cin, cout, nch, ks,
                                                                                        ntp);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// the instance norm's gradient and the bias gradient
// ---------------------------------------------------------------------------------------------------------------
constexpr int NG_CHUNK = DVC_ENC_GRAD_CHUNK;
static_assert(NG_CHUNK == 4096, "256 threads x 16 values");

// the four waves' double sums, in wave order, to thread 0
__device__ __forceinline__ double ng_block_sum(double v, double *sm, int tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((tid & 63) == 0) sm[tid >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// grid (chunk, plane = b C + c); part[plane][chunk][3]: sum gn, sum gn n (k_enc_ng_sums), sum g_x (k_enc_ng_apply)
__global__ __launch_bounds__(256) void k_enc_ng_sums(const float *__restrict__ g, const float *__restrict__ x,
                                                     const float *__restrict__ ss, int mask, double *__restrict__ part,
                                                     long long HWD, int nchunk) {
    __shared__ double sm1[4], sm2[4];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const long long plane = blockIdx.y, row = plane * HWD, start = (long long)chunk * NG_CHUNK;
    const float a = ss[2 * plane], sh = ss[2 * plane + 1];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const long long idx = start + i * 256 + tid;
        if (idx < HWD) {
            const float n = fmaf(x[row + idx], a, sh);
            const float gn = mask && !(n > 0.0f) ? 0.0f : g[row + idx];
            s1 += (double)gn;
            s2 += (double)gn * (double)n;
        }
    }
    s1 = ng_block_sum(s1, sm1, tid);
    s2 = ng_block_sum(s2, sm2, tid);
    if (tid == 0) {
        double *p = part + (plane * nchunk + chunk) * 3;
        p[0] = s1;
        p[1] = s2;
    }
}

__global__ __launch_bounds__(256) void k_enc_ng_apply(const float *__restrict__ g, const float *__restrict__ x,
                                                      const float *__restrict__ ss, int mask, float *__restrict__ gx,
                                                      double *__restrict__ part, long long HWD, int nchunk) {
    __shared__ double sm[4];
    __shared__ float mm[2];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const long long plane = blockIdx.y, row = plane * HWD, start = (long long)chunk * NG_CHUNK;
    float a = 1.0f, sh = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if (ss) {
        a = ss[2 * plane];
        sh = ss[2 * plane + 1];
        if (tid == 0) {
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < nchunk; ++k) {
                s1 += part[(plane * nchunk + k) * 3];
                s2 += part[(plane * nchunk + k) * 3 + 1];
            }
            mm[0] = (float)(s1 / (double)HWD);
            mm[1] = (float)(s2 / (double)HWD);
        }
        __syncthreads();
        m1 = mm[0];
        m2 = mm[1];
    }
    double sb = 0.0;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const long long idx = start + i * 256 + tid;
        if (idx < HWD) {
            float v = g[row + idx];
            if (ss) {
                const float n = fmaf(x[row + idx], a, sh);
                if (mask && !(n > 0.0f)) v = 0.0f;
                v = a * ((v - m1) - n * m2);
            } else if (mask && !(x[row + idx] > 0.0f)) {
                v = 0.0f;
            }
            if (gx) gx[row + idx] = v;
            sb += (double)v;
        }
    }
    sb = ng_block_sum(sb, sm, tid);
    if (tid == 0) part[(plane * nchunk + chunk) * 3 + 2] = sb;
}

__global__ __launch_bounds__(128) void k_enc_db_reduce(const double *__restrict__ part, float *__restrict__ db, int C,
                                                       int B, int nchunk) {
    const int c = blockIdx.x * 128 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nchunk; ++k) s += part[(((long long)b * C + c) * nchunk + k) * 3 + 2];
    db[c] = (float)s;
}

size_t enc_grad_partials_bytes(int C, int B, long long HWD) {
    return (size_t)B * C * ((HWD + NG_CHUNK - 1) / NG_CHUNK) * 3 * sizeof(double);
}

// host entry: arguments validated by dvc_enc_norm_grad (capi.hip)
hipError_t launch_enc_norm_grad(const float *g, const float *x, const float *scale_shift, int mask, float *gx, float *db,
                                void *partials, int C, int B, long long HWD, hipStream_t s) {
    const int nchunk = (int)((HWD + NG_CHUNK - 1) / NG_CHUNK);
    const dim3 grid((unsigned)nchunk, (unsigned)(B * C));
    double *part = static_cast<double *>(partials);
    if (scale_shift) k_enc_ng_sums<<<grid, 256, 0, s>>>(g, x, scale_shift, mask, part, HWD, nchunk);
    k_enc_ng_apply<<<grid, 256, 0, s>>>(g, x, scale_shift, mask, gx, part, HWD, nchunk);
    if (db) k_enc_db_reduce<<<(unsigned)((C + 127) / 128), 128, 0, s>>>(part, db, C, B, nchunk);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// elementwise: the residual's gradient sum and conv2's tanh / ReLU split
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_enc_grad_add(const float *__restrict__ a, const float *__restrict__ b,
                                                      const float *__restrict__ m, float *__restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v = a[i];
        if (b) v += b[i];
        if (m && !(m[i] > 0.0f)) v = 0.0f;
        dst[i] = v;
    }
}

hipError_t launch_enc_grad_add(const float *a, const float *b, const float *m, float *dst, long long n, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    k_enc_grad_add<<<grid, 256, 0, s>>>(a, b, m, dst, n);
    return hipGetLastError();
}

// g (B, cout, V): channels [0, split) g_net (1 - net^2), the rest g_ctx [ctx > 0]; a null gradient is zero
__global__ __launch_bounds__(256) void k_enc_split_grad(const float *__restrict__ g_net, const float *__restrict__ g_ctx,
                                                        const float *__restrict__ net, const float *__restrict__ ctx,
                                                        float *__restrict__ g, int split, int cout, long long V,
                                                        long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long plane = i / V, v = i - plane * V;
        const int b = (int)(plane / cout), c = (int)(plane - (long long)b * cout);
        float r;
        if (c < split) {
            const long long k = ((long long)b * split + c) * V + v;
            const float t = net[k];
            r = g_net ? g_net[k] * (1.0f - t * t) : 0.0f;
        } else {
            const long long k = ((long long)b * (cout - split) + (c - split)) * V + v;
            r = g_ctx && ctx[k] > 0.0f ? g_ctx[k] : 0.0f;
        }
        g[i] = r;
    }
}

hipError_t launch_enc_split_grad(const float *g_net, const float *g_ctx, const float *net, const float *ctx, float *g,
                                 int split, int cout, int B, long long V, hipStream_t s) {
    const long long n = (long long)B * cout * V;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    k_enc_split_grad<<<grid, 256, 0, s>>>(g_net, g_ctx, net, ctx, g, split, cout, V, n);
    return hipGetLastError();
}

}  // namespace dvc
