// conv7_grad.hip -- the weight gradient of k_conv7_flow (conv3.hip): what encoder.convf1 (3 -> 64, 7 x 7 x 7, + bias
// + ReLU) needs to train.  With g = dL/dy [y > 0] (k_conv3_grad_prep, conv3_grad.hip, which also sums db):
//   dW[o][ci][kh][kw][kd] = sum over (b, h, w, d) of g[b, o, h, w, d] flow[b, ci, h + kh - 3, w + kw - 3, d + kd - 3],
// out-of-volume flow counting as zero.  The layer's input is the flow, which the model detaches at every iteration
// (raft_dvc.py:441), so no input gradient is computed here.
//
// k_conv7_wgrad.  A GEMM whose K runs over the voxels, on v_mfma_f32_16x16x32 with M = output channels (A operand = g)
// and N = the flat weight index n = (ci 7 + kh) 49 + kw 7 + kd (B operand = flow): 1029 columns in 65 tiles of 16, the
// columns past 1029 zeros.  A workgroup (four waves) owns DVC_CONV7_WGRAD_TILES consecutive N tiles x all four o
// tiles, over a slab of K-blocks; a K-block is the forward's 4 x 4 x 16 voxel box.
//   stage    per K-block the 10 x 10 x 22 flow halo of the three channels goes to LDS in float32, as k_conv7_flow
//            stages it, and g as [64 o][256 voxels] rows of 16-bit values (k_conv3_wgrad's pitch rule: 16 bytes past a
//            multiple of 256).  Out-of-volume voxels are zeros.  The next K-block's global loads are in flight under
//            the current block's MFMAs.
//   MFMA     one K = 32 step is two columns adjacent along W x 16 d: lane group h4 holds column h4 >> 1, d values
//            8 (h4 & 1) .. + 7.  The A operand is one ds_read_b128.  The B operand of column n is eight consecutive d
//            values of flow channel ci at offset (kh, kw, kd): eight dword LDS reads and split2, as the forward builds
//            its runs.  A built B fragment serves all four o tiles and all pieces.
//   split    the waves deal K: wave w owns the box's row bh = w (two K steps).  The four partial sums meet once per
//            workgroup, through LDS, in wave order.
//   split-K  the grid is N-tile groups x slabs; a slab is `per` consecutive K-blocks of the (B, H, W, D) box grid,
//            per = ceil(nbox / min(nbox, ceil(TARGET / groups))), and only the ceil(nbox / per) slabs that hold a box
//            are launched.  A workgroup writes its partial dW to the workspace [slab][64][1029];
//            k_conv3_wgrad_reduce sums the slabs in index order.
// Precisions as the forward: T = bf16 / fp16, NP = 1: both operands rounded once, fp32 accumulation; fp32 (T = bf16,
// NP = 2): bf16 hi + lo pieces, g_lo x_hi + g_hi x_lo + g_hi x_hi.
//
// No atomics, no allocation or synchronisation on the host; every sum has a fixed order.
#include "mfma_conv.h"

namespace dvc {

hipError_t launch_wgrad_reduce(const float *ws, float *dw, int n, int nslab, hipStream_t s);   // conv3_grad.hip

constexpr int W7_KH = DVC_CONV7_WGRAD_KH, W7_KW = DVC_CONV7_WGRAD_KW, W7_KD = DVC_CONV7_WGRAD_KD;
constexpr int W7_NG = DVC_CONV7_WGRAD_TILES;                // N tiles per workgroup
constexpr int W7_COUT = DVC_CONV7_COUT;
constexpr int W7_N = 3 * 343;                               // 1029 weights per output channel
constexpr int W7_NTILES = (W7_N + 15) / 16;                 // 65
constexpr int W7_GROUPS = (W7_NTILES + W7_NG - 1) / W7_NG;  // 13
static_assert(W7_KH == 4 && W7_KW == 4 && W7_KD == 16 && W7_COUT == 64,
              "four waves x two K = 32 steps of two columns x 16 d; four o tiles");
constexpr int W7_HW = W7_KW + 6, W7_HD = W7_KD + 8;         // D pitch: 22 halo values + 2 zeros, as k_conv7_flow
constexpr int W7_CH = (W7_KH + 6) * W7_HW * W7_HD;          // 2400 floats per channel
constexpr int W7_XIT = (3 * W7_CH + 255) / 256;             // flow halo values per staging thread
constexpr int W7_GPITCH = W7_KH * W7_KW * W7_KD * 2 + 16;   // a g row: 256 voxels of 16 bits, + 16 bytes
constexpr int W7_GIT = W7_COUT / 2;                         // g pairs per staging thread
static_assert(W7_GPITCH % 256 == 16, "b128 reads of 16 channels: distinct 16-byte slots");

struct Wgrad7Args {
    const float *flow, *g;
    float *ws;
    long long HWD;
    int B, H, W, D, nth, ntw, ntd, nbox, per, nslab;
};

// the slab rule (see the head of this file)
static void wgrad7_slabs(int B, int H, int W, int D, int &nbox, int &per, int &nslab) {
    const long long nb = (long long)B * ((H + W7_KH - 1) / W7_KH) * ((W + W7_KW - 1) / W7_KW) * ((D + W7_KD - 1) / W7_KD);
    long long want = (DVC_CONV7_WGRAD_TARGET + W7_GROUPS - 1) / W7_GROUPS;
    if (want > nb) want = nb;
    nbox = (int)nb;
    per = (int)((nb + want - 1) / want);
    nslab = (int)((nb + per - 1) / per);
}

size_t conv7_wgrad_workspace_bytes(int B, int H, int W, int D) {
    int nbox, per, nslab;
    wgrad7_slabs(B, H, W, D, nbox, per, nslab);
    return (size_t)nslab * W7_COUT * W7_N * sizeof(float);
}

template <typename T, int NP>
__global__ __launch_bounds__(256, 1) void k_conv7_wgrad(Wgrad7Args A) {
    constexpr int GPIECE = W7_COUT * W7_GPITCH;
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * GPIECE + 3 * W7_CH * 4];
    static_assert(NP * GPIECE >= 4 * 4 * 1024, "the epilogue's exchange buffer");
    unsigned char *gs = smem;
    float *xs = reinterpret_cast<float *>(smem + NP * GPIECE);
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = (int)(blockIdx.x % (unsigned)A.nslab), grp = (int)(blockIdx.x / (unsigned)A.nslab);
    const long long HWD = A.HWD;

    // g staging: this thread's pair (d, d + 1) of column (gbh, gbw), channels go + 2 i
    const int gq = tid & 127, gbh = gq >> 5, gbw = (gq >> 3) & 3, gd = 2 * (gq & 7), go = tid >> 7;
    float gv[W7_GIT][2], xv[W7_XIT];

    auto stage_load = [&](int bx) __attribute__((always_inline)) {
        int b, h0, w0, d0;
        box_of_block((unsigned)bx, A.nth, A.ntw, A.ntd, W7_KH, W7_KW, W7_KD, b, h0, w0, d0);
        {
            const int h = h0 + gbh, w = w0 + gbw, d = d0 + gd;
            const bool ok0 = h < A.H && w < A.W && d < A.D, ok1 = ok0 && d + 1 < A.D;
            const float *gb = A.g + (long long)b * W7_COUT * HWD + ((long long)h * A.W + w) * A.D + d;
#pragma unroll
            for (int i = 0; i < W7_GIT; ++i) {
                const int o = go + 2 * i;
                gv[i][0] = ok0 ? gb[(long long)o * HWD] : 0.0f;
                gv[i][1] = ok1 ? gb[(long long)o * HWD + 1] : 0.0f;
            }
        }
        const float *src = A.flow + (long long)b * 3 * HWD;
#pragma unroll
        for (int k = 0; k < W7_XIT; ++k) {
            const int i = tid + 256 * k;
            const int ci = i / W7_CH, r = i - ci * W7_CH;
            const int hh = r / (W7_HW * W7_HD), rem = r - hh * (W7_HW * W7_HD), ww = rem / W7_HD, dd = rem - ww * W7_HD;
            const int h = h0 - 3 + hh, w = w0 - 3 + ww, d = d0 - 3 + dd;
            const bool ok = i < 3 * W7_CH && dd < W7_KD + 6 && h >= 0 && h < A.H && w >= 0 && w < A.W && d >= 0 && d < A.D;
            xv[k] = ok ? src[(long long)ci * HWD + ((long long)h * A.W + w) * A.D + d] : 0.0f;
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < W7_GIT; ++i) {
            unsigned hi, lo;
            split2<T, NP>(gv[i][0], gv[i][1], hi, lo);
            unsigned char *p = gs + (go + 2 * i) * W7_GPITCH + gq * 4;
            *reinterpret_cast<unsigned *>(p) = hi;
            if constexpr (NP == 2) *reinterpret_cast<unsigned *>(p + GPIECE) = lo;
        }
#pragma unroll
        for (int k = 0; k < W7_XIT; ++k) {
            const int i = tid + 256 * k;
            if (i < 3 * W7_CH) xs[i] = xv[k];
        }
    };

    // this lane's weight columns: n = 16 (W7_NG grp + j) + m16 -> the halo offset of (ci, kh, kw, kd)
    int noff[W7_NG];
    bool nok[W7_NG];
#pragma unroll
    for (int j = 0; j < W7_NG; ++j) {
        const int n = 16 * (W7_NG * grp + j) + m16;
        nok[j] = n < W7_N;
        const int nn = nok[j] ? n : 0;
        const int ci = nn / 343, t = nn - 343 * ci, kh = t / 49, kw = (t - 49 * kh) / 7, kd = t - 49 * kh - 7 * kw;
        noff[j] = ci * W7_CH + (kh * W7_HW + kw) * W7_HD + kd;
    }

    f32x4 acc[W7_NG][4];
#pragma unroll
    for (int j = 0; j < W7_NG; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane (m16, h4): A = g row of channel m16 of each o tile; column h4 >> 1 of the pair, d half h4 & 1
    const unsigned char *ga = gs + m16 * W7_GPITCH + wave * (W7_KW * W7_KD * 2) + h4 * 16;
    const float *xb = xs + (wave * W7_HW + (h4 >> 1)) * W7_HD + (h4 & 1) * 8;

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
            u32x4 af[4][NP];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
                    af[t][pc] = *reinterpret_cast<const u32x4 *>(ga + pc * GPIECE + t * 16 * W7_GPITCH + p * 64);
            const float *xp = xb + 2 * p * W7_HD;
#pragma unroll
            for (int j = 0; j < W7_NG; ++j) {
                float f[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) f[k] = nok[j] ? xp[noff[j] + k] : 0.0f;
                unsigned hi[4], lo[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) split2<T, NP>(f[2 * k], f[2 * k + 1], hi[k], lo[k]);
                u32x4 bf[NP];
                bf[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
                if constexpr (NP == 2) bf[1] = u32x4{lo[0], lo[1], lo[2], lo[3]};
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[j][t] = mma_step<T, NP>(af[t], bf, acc[j][t]);
            }
        }
    }

    // the four waves' partial sums meet in LDS, one N tile (four accumulators) per round, summed in wave order.  Lane
    // (m16, h4) holds weight column 16 tile + m16, output channels 16 t + 4 h4 + k.
    float *red = reinterpret_cast<float *>(smem);
    float *wsl = A.ws + (long long)slab * W7_COUT * W7_N;
    const int rl = tid >> 2, rk = tid & 3;
#pragma unroll
    for (int j = 0; j < W7_NG; ++j) {
        const int rn = 16 * (W7_NG * grp + j) + (rl & 15);
        __syncthreads();   // the main loop's reads, or the previous round's, are done
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4 *>(red + ((wave * 4 + t) * 64 + lane) * 4) = acc[j][t];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float s = ((red[t * 256 + tid] + red[1024 + t * 256 + tid]) + red[2048 + t * 256 + tid]) +
                            red[3072 + t * 256 + tid];
            const int ro = 16 * t + 4 * (rl >> 4) + rk;
            if (rn < W7_N) wsl[(long long)ro * W7_N + rn] = s;
        }
    }
}

// host entry: arguments validated by dvc_conv7_wgrad (capi.hip)
hipError_t launch_conv7_wgrad(const float *flow, const float *g, float *dw, void *workspace, int B, int H, int W, int D,
                              int dtype, hipStream_t s) {
    Wgrad7Args A;
    A.flow = flow; A.g = g; A.ws = static_cast<float *>(workspace);
    A.HWD = (long long)H * W * D;
    A.B = B; A.H = H; A.W = W; A.D = D;
    A.nth = (H + W7_KH - 1) / W7_KH; A.ntw = (W + W7_KW - 1) / W7_KW; A.ntd = (D + W7_KD - 1) / W7_KD;
    wgrad7_slabs(B, H, W, D, A.nbox, A.per, A.nslab);
    const unsigned grid = (unsigned)(A.nslab * W7_GROUPS);
    with_precision(dtype, [&](auto t, auto np) {
        k_conv7_wgrad<decltype(t), decltype(np)::value><<<grid, 256, 0, s>>>(A);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wgrad_reduce(A.ws, dw, W7_COUT * W7_N, A.nslab, s);
}

}  // namespace dvc
