// gru_grad.hip -- the backward of k_sep_gru_pass (gru.hip): what one axis pass of SepConvGRU3D needs to train (the
// autograd formula of dvccorr::sep_gru_ad, dvccorr/library.py).  The training forward (k_sep_gru_pass<.., SAVE>) stores
// z, r and q (after tanh) of every voxel.  With G = dL/dh' and *T the 5-tap transposed convolution along the pass axis,
// zero padding 2:
//     a_q = G z (1 - q^2)             a_z = G (q - h) z (1 - z)
//     D   = Wq^T *T a_q               (96 + Cx channels: d(r h) = D[:96], dx += D[96:])
//     a_r = D[:96] h r (1 - r)
//     E   = [Wz; Wr]^T *T [a_z; a_r]  (96 + Cx channels)
//     dh  = G (1 - z) + D[:96] r + E[:96]        dx += E[96:]
//     dW_g[o][ci][t] = sum over (b, v) of a_g[b, o, v] in_g[b, ci, v + (t - 2) e_axis], in_z = in_r = cat[h, x],
//     in_q = cat[r h, x];  db_g[o] = sum over (b, v) of a_g[b, o, v]
//
// k_gru_grad_prep   one streaming pass over G, z, q, h: a_q, a_z, dh0 = G (1 - z) and the per-workgroup partial sums of
//                   db_q and db_z (the pattern of k_conv3_grad_prep); k_gru_db_reduce adds a channel's partials in
//                   index order.  db_r is conv3_grad.hip's prep kernel on the stored a_r.
// k_sep_gru_dgrad   the transposed convolution as k_sep_gru_pass's implicit GEMM: a workgroup (four waves) owns
//                   S = DVC_GRU_SEG positions of 16 lines and all sixteen 16-channel tiles of the 96 + Cx outputs padded
//                   to 256; wave w owns positions 2 w, 2 w + 1 (32 accumulators).  The operand is staged as the
//                   forward's rows of 32 channels (S + 4 positions), the next chunk's loads in flight under the current
//                   chunk's MFMAs; the weights are the fragments of W'[ci][o][t'] = W[o][ci][4 - t'] (k_gru_pack_dgrad).
//                   Two launches per pass: the q stage (K = 5 x 96: a_q) writes a_r, dh = dh0 + D[:96] r and
//                   dx (=, +=) D[96:]; the z/r stage (K = 5 x 192: a_z, a_r) adds E[:96] to dh and E[96:] to dx.  The
//                   split is there because a_r at the S + 4 halo positions needs D at positions other workgroups own:
//                   fusing both stages means recomputing D on an S + 8 halo.  A position belongs to
//                   one workgroup: no atomics.
// k_gru_wgrad       dW as a split-K GEMM over the voxels: M = the 96 rows of one gate's a_g, N = one 16-channel tile of
//                   the 256 padded input channels, five tap accumulators per (o tile, ci tile): 30 per wave.  A K-block
//                   is DVC_GRU_WGRAD_LINES lines x DVC_GRU_WGRAD_POS positions; K of one MFMA is the 32 lines of one
//                   position, so a tap is another row of the staged image and one image serves all five taps.  Both
//                   operands sit in LDS as 16-bit rows [channel][position][32 lines], the 16-byte slots of a row
//                   XOR-swizzled by the channel so that a ds_read_b128 of 16 channels is conflict-free.  Wave w owns
//                   position w of the block; the four partial sums meet through LDS in wave order.  Slabs of
//                   consecutive K-blocks go to a workspace and are summed in index order (conv3_grad.hip's rule and
//                   reduce kernel).
// Precisions as the forward: T = bf16 / fp16, NP = 1: both operands rounded once, fp32 accumulation; fp32 (T = bf16,
// NP = 2): bf16 hi + lo pieces, three MFMAs per step.  No atomics, no allocation or synchronisation on the host.
#include "mfma_conv.h"

namespace dvc {

hipError_t launch_conv3_grad_prep(const float *grad_y, const float *y, float *g, float *db, float *partial, int cout,
                                  int B, int H, int W, int D, hipStream_t s);
hipError_t launch_wgrad_reduce(const float *ws, float *dw, int n, int nslab, hipStream_t s);

constexpr int GG_S = DVC_GRU_SEG, GG_HID = DVC_GRU_HIDDEN;
constexpr int GG_FRAGS_Q = 3 * 5 * 16, GG_FRAGS_ZR = 6 * 5 * 16;   // 1 KB fragments per piece of the two stages
constexpr int GP_CHUNK = DVC_CONV3_PREP_CHUNK;
constexpr int GW_P = DVC_GRU_WGRAD_POS, GW_L = DVC_GRU_WGRAD_LINES;
static_assert(GP_CHUNK == 4096, "256 threads x 4 float4");
static_assert(GW_P == 4 && GW_L == 32, "four waves, one position each; K = 32 lines");

// the geometry of one axis pass
struct GruGeom {
    long long HWD, pstride;   // channel stride; stride of one step along the conv axis
    int B, Cx, H, W, D, axis, len, nlines, per_b;
};

static GruGeom gru_geom(int B, int Cx, int H, int W, int D, int axis) {
    GruGeom G;
    G.B = B; G.Cx = Cx; G.H = H; G.W = W; G.D = D; G.axis = axis;
    G.HWD = (long long)H * W * D;
    G.len = axis == 0 ? H : axis == 1 ? W : D;
    G.pstride = axis == 0 ? (long long)W * D : axis == 1 ? D : 1;
    G.per_b = (int)(G.HWD / G.len);
    G.nlines = B * G.per_b;
    return G;
}

// ---------------------------------------------------------------------------------------------------------------
// k_gru_grad_prep.  Workgroup (chunk, o, b) owns GP_CHUNK consecutive voxels of channel o of batch element b; a thread
// sums its values in index order, a wave by a shuffle tree, the four waves in wave order:
// partial[gate q, z][o][b][chunk].
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gru_prep_one(float g, float z, float q, float h, float &aq, float &az, float &dh) {
    aq = (g * z) * (1.0f - q * q);
    az = (g * (q - h)) * (z * (1.0f - z));
    dh = g * (1.0f - z);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_gru_grad_prep(const float *__restrict__ g, const float *__restrict__ z,
                                                       const float *__restrict__ q, const float *__restrict__ h,
                                                       float *__restrict__ aq, float *__restrict__ az,
                                                       float *__restrict__ dh, float *__restrict__ partial,
                                                       long long HWD, int B, int nchunk) {
    __shared__ float wsum[2][4];
    const int tid = threadIdx.x, chunk = blockIdx.x, o = blockIdx.y, b = blockIdx.z;
    const long long row = ((long long)b * GG_HID + o) * HWD, start = (long long)chunk * GP_CHUNK;
    float sq = 0.0f, sz = 0.0f;
    if constexpr (VEC) {   // HWD is a multiple of four and the pointers are 16-byte aligned
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long idx = start + (long long)(i * 256 + tid) * 4;
            if (idx < HWD) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + row + idx);
                const f32x4 zv = *reinterpret_cast<const f32x4 *>(z + row + idx);
                const f32x4 qv = *reinterpret_cast<const f32x4 *>(q + row + idx);
                const f32x4 hv = *reinterpret_cast<const f32x4 *>(h + row + idx);
                f32x4 a, c, d;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float ak, ck, dk;
                    gru_prep_one(gv[k], zv[k], qv[k], hv[k], ak, ck, dk);
                    a[k] = ak;
                    c[k] = ck;
                    d[k] = dk;
                }
                *reinterpret_cast<f32x4 *>(aq + row + idx) = a;
                *reinterpret_cast<f32x4 *>(az + row + idx) = c;
                *reinterpret_cast<f32x4 *>(dh + row + idx) = d;
                sq += (a[0] + a[1]) + (a[2] + a[3]);
                sz += (c[0] + c[1]) + (c[2] + c[3]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long idx = start + i * 256 + tid;
            if (idx < HWD) {
                float a, c, d;
                gru_prep_one(g[row + idx], z[row + idx], q[row + idx], h[row + idx], a, c, d);
                aq[row + idx] = a;
                az[row + idx] = c;
                dh[row + idx] = d;
                sq += a;
                sz += c;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sq += __shfl_down(sq, d, 64);
        sz += __shfl_down(sz, d, 64);
    }
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = sq;
        wsum[1][tid >> 6] = sz;
    }
    __syncthreads();
    if (tid < 2)
        partial[(((long long)tid * GG_HID + o) * B + b) * nchunk + chunk] =
            ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
}

// db_q[o], db_z[o] = the channel's n partials, summed in index order
__global__ __launch_bounds__(64) void k_gru_db_reduce(const float *__restrict__ partial, float *__restrict__ dbq,
                                                      float *__restrict__ dbz, int n) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= 2 * GG_HID) return;
    float s = 0.0f;
    for (int k = 0; k < n; ++k) s += partial[(long long)o * n + k];
    if (o < GG_HID) dbq[o] = s;
    else dbz[o - GG_HID] = s;
}

// host entry: arguments validated by dvc_gru_grad_prep (capi.hip)
hipError_t launch_gru_grad_prep(const float *g, const float *z, const float *q, const float *h, float *aq, float *az,
                                float *dh, float *dbq, float *dbz, float *partial, int B, int H, int W, int D,
                                hipStream_t s) {
    const long long HWD = (long long)H * W * D;
    const int nchunk = (int)((HWD + GP_CHUNK - 1) / GP_CHUNK);
    const dim3 grid((unsigned)nchunk, (unsigned)GG_HID, (unsigned)B);
    const uintptr_t al = (uintptr_t)g | (uintptr_t)z | (uintptr_t)q | (uintptr_t)h | (uintptr_t)aq | (uintptr_t)az |
                         (uintptr_t)dh;
    if (HWD % 4 == 0 && al % 16 == 0) k_gru_grad_prep<true><<<grid, 256, 0, s>>>(g, z, q, h, aq, az, dh, partial, HWD, B, nchunk);
    else k_gru_grad_prep<false><<<grid, 256, 0, s>>>(g, z, q, h, aq, az, dh, partial, HWD, B, nchunk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_gru_db_reduce<<<(2 * GG_HID + 63) / 64, 64, 0, s>>>(partial, dbq, dbz, B * nchunk);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// k_sep_gru_dgrad
// ---------------------------------------------------------------------------------------------------------------
struct GruDgradArgs {
    GruGeom G;
    const float *in0, *in1;   // the stage's operand: chunks 0..2 (a_q; a_z), chunks 3..5 (a_r)
    const float *h, *r;       // q stage: the pass's input hidden state and reset gate
    const unsigned char *w;   // the stage's fragments (k_gru_pack_dgrad)
    float *ar, *dh, *dx;      // dx may be null (no input gradient asked for)
    int ntiles, dx_add;       // output tiles computed (6 without dx); dx += instead of dx =
};

template <typename T, int NP, int NCH, bool QS>
__global__ __launch_bounds__(256, 1) void k_sep_gru_dgrad(GruDgradArgs A) {
    constexpr int S = GG_S, ROWB = kRowBytes, PIECE = 16 * 16 * ROWB, NUNITS = NCH * 5 * 2;
    static_assert(S == 8, "four waves x two positions; 256 threads stage 16 positions x 16 lines, S + 4 of them used");
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * PIECE];
    const GruGeom &G = A.G;
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nlg = (G.nlines + 15) / 16;
    const int lg = (int)(blockIdx.x % (unsigned)nlg), seg0 = (int)(blockIdx.x / (unsigned)nlg) * S;
    const long long HWD = G.HWD;

    // the voxel this thread stages (row sp = position seg0 - 2 + sp): consecutive lanes walk the contiguous direction
    const int sline = G.axis == 2 ? tid >> 4 : tid & 15;
    const int sp = G.axis == 2 ? tid & 15 : tid >> 4;
    int sb;
    long long soff;
    bool sok = gru_line(G, lg * 16 + sline, sb, soff);
    const int spos = seg0 - 2 + sp;
    sok = sok && sp < S + 4 && spos >= 0 && spos < G.len;
    if (!sok) { sb = 0; soff = 0; } else soff += (long long)spos * G.pstride;
    const float *s0 = A.in0 + (long long)sb * GG_HID * HWD + soff;
    const float *s1 = A.in1 + (long long)sb * GG_HID * HWD + soff;
    unsigned char *srow = smem + (sp * 16 + sline) * ROWB;

    // the line of this lane's MFMA column
    int mb;
    long long moff;
    const bool mok = gru_line(G, lg * 16 + m16, mb, moff);

    float st[32];
    auto stage_load = [&](int c) __attribute__((always_inline)) {
        const float *p = (c < 3 ? s0 : s1) + (long long)(32 * (c < 3 ? c : c - 3)) * HWD;
#pragma unroll
        for (int k = 0; k < 32; ++k) st[k] = sok ? p[(long long)k * HWD] : 0.0f;
    };

    f32x4 acc[16][2];
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 wc[8][NP], wn[8][NP];
    const unsigned char *wb = A.w + lane * 16;
    int u = 0;
    load_frags(wb, 0, NUNITS, 8, wc);
    stage_load(0);
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
        __syncthreads();   // the previous chunk's reads are done
        stage_row<T, NP>(st, srow, PIECE);
        __syncthreads();
        if (c + 1 < NCH) stage_load(c + 1);
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            u32x4 bf[2][NP];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
                    bf[i][pc] = *reinterpret_cast<const u32x4 *>(smem + pc * PIECE +
                                                                 ((2 * wave + i + t) * 16 + m16) * ROWB + h4 * 16);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                ++u;
                load_frags(wb, u, NUNITS, 8, wn);   // the next unit's fragments, in flight under this unit's MFMAs
#pragma unroll
                for (int tl = 0; tl < 8; ++tl)
                    if (hf * 8 + tl < A.ntiles) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) acc[hf * 8 + tl][i] = mma_step<T, NP>(wc[tl], bf[i], acc[hf * 8 + tl][i]);
                    }
#pragma unroll
                for (int tl = 0; tl < 8; ++tl)
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc) wc[tl][pc] = wn[tl][pc];
            }
        }
    }

    // epilogue: lane (m16, h4) holds line m16, channels 16 tile + 4 h4 + k of its two positions
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pos = seg0 + 2 * wave + i;
        if (!(mok && pos < G.len)) continue;
        const long long voff = moff + (long long)pos * G.pstride;
        const long long hb = (long long)mb * GG_HID * HWD + voff;
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long idx = hb + (long long)(16 * t + 4 * h4 + k) * HWD;
                const float v = acc[t][i][k];
                if constexpr (QS) {
                    const float hv = A.h[idx], rv = A.r[idx];
                    A.ar[idx] = (v * hv) * (rv * (1.0f - rv));
                    A.dh[idx] = A.dh[idx] + v * rv;
                } else {
                    A.dh[idx] = A.dh[idx] + v;
                }
            }
        if (A.dx) {
            float *dxb = A.dx + (long long)mb * G.Cx * HWD + voff;
#pragma unroll
            for (int t = 6; t < 16; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = 16 * t + 4 * h4 + k - GG_HID;
                    if (cx < G.Cx) {
                        float *p = dxb + (long long)cx * HWD;
                        *p = A.dx_add ? *p + acc[t][i][k] : acc[t][i][k];
                    }
                }
        }
    }
}

// Packed input-gradient weights of one axis: the q stage's fragments [chunk c of Wq's 96 rows][tap t'][16 tiles], then
// the z/r stage's [chunk c of the 192 rows of (Wz; Wr)][tap t'][16 tiles]; each fragment NP pieces of [lane][8] 16-bit
// values, lane l element j = W[row 32 c + 8 (l >> 4) + j][padded input channel 16 tile + (l & 15)][4 - t'].
template <typename T, int NP>
__global__ __launch_bounds__(256) void k_gru_pack_dgrad(const float *__restrict__ wz, const float *__restrict__ wr,
                                                        const float *__restrict__ wq, unsigned char *__restrict__ out,
                                                        int Cx) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (GG_FRAGS_Q + GG_FRAGS_ZR) * 512) return;
    int fr, l, j;
    frag_elem(e, fr, l, j);
    const int f = fr < GG_FRAGS_Q ? fr : fr - GG_FRAGS_Q;
    const int c = f / 80, t = (f % 80) / 16, tile = f % 16;
    const int row = 32 * c + 8 * (l >> 4) + j, co = 16 * tile + (l & 15), cin = GG_HID + Cx;
    const float *w = fr < GG_FRAGS_Q ? wq : row < GG_HID ? wz : wr;
    const int o = row < GG_HID ? row : row - GG_HID;
    pack_store<T, NP>(out, fr, l, j, co < cin ? w[((long long)o * cin + co) * 5 + 4 - t] : 0.0f);
}

size_t gru_dgrad_packed_bytes(int dtype) { return (size_t)(GG_FRAGS_Q + GG_FRAGS_ZR) * pieces_of(dtype) * kFragBytes; }

hipError_t launch_gru_pack_dgrad(const float *wz, const float *wr, const float *wq, void *packed, int Cx, int dtype,
                                 hipStream_t s) {
    const unsigned blocks = (GG_FRAGS_Q + GG_FRAGS_ZR) * 512 / 256;
    unsigned char *out = static_cast<unsigned char *>(packed);
    with_precision(dtype, [&](auto t, auto np) {
        k_gru_pack_dgrad<decltype(t), decltype(np)::value><<<blocks, 256, 0, s>>>(wz, wr, wq, out, Cx);
    });
    return hipGetLastError();
}

// host entry: arguments validated by dvc_sep_gru_dgrad (capi.hip); dx may be null
hipError_t launch_sep_gru_dgrad(const float *aq, const float *az, const float *h, const float *r, const void *packed,
                                float *ar, float *dh, float *dx, float *dbr, float *partial, int B, int Cx, int H, int W,
                                int D, int axis, int dx_add, int dtype, hipStream_t s) {
    GruDgradArgs A;
    A.G = gru_geom(B, Cx, H, W, D, axis);
    A.h = h; A.r = r; A.ar = ar; A.dh = dh; A.dx = dx;
    A.ntiles = dx ? (GG_HID + Cx + 15) / 16 : GG_HID / 16;
    const unsigned grid = (unsigned)((A.G.nlines + 15) / 16) * (unsigned)((A.G.len + GG_S - 1) / GG_S);
    const unsigned char *w = static_cast<const unsigned char *>(packed);
    const size_t zr_off = (size_t)GG_FRAGS_Q * pieces_of(dtype) * kFragBytes;
    A.in0 = aq; A.in1 = aq; A.w = w; A.dx_add = dx_add;
    with_precision(dtype, [&](auto t, auto np) {
        k_sep_gru_dgrad<decltype(t), decltype(np)::value, 3, true><<<grid, 256, 0, s>>>(A);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    A.in0 = az; A.in1 = ar; A.w = w + zr_off; A.dx_add = 1;
    with_precision(dtype, [&](auto t, auto np) {
        k_sep_gru_dgrad<decltype(t), decltype(np)::value, 6, false><<<grid, 256, 0, s>>>(A);
    });
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_conv3_grad_prep(ar, nullptr, nullptr, dbr, partial, GG_HID, B, H, W, D, s);
}

// ---------------------------------------------------------------------------------------------------------------
// k_gru_wgrad
// ---------------------------------------------------------------------------------------------------------------
struct GruWgradArgs {
    GruGeom G;
    const float *h, *x, *r, *az, *ar, *aq;
    float *ws;
    int ncit, npb, nkb, per, nslab;
};

// the slab rule (conv3_grad.hip's, over the K-blocks of this kernel)
static void gru_wgrad_slabs(int Cx, int B, int H, int W, int D, int axis, int &npb, int &nkb, int &per, int &nslab) {
    const GruGeom G = gru_geom(B, Cx, H, W, D, axis);
    npb = (G.len + GW_P - 1) / GW_P;
    const long long nb = (long long)((G.nlines + GW_L - 1) / GW_L) * npb;
    const long long tiles = 3LL * ((GG_HID + Cx + 15) / 16);
    long long want = (DVC_GRU_WGRAD_TARGET + tiles - 1) / tiles;
    if (want > nb) want = nb;
    nkb = (int)nb;
    per = (int)((nb + want - 1) / want);
    nslab = (int)((nb + per - 1) / per);
}

size_t gru_wgrad_workspace_bytes(int Cx, int B, int H, int W, int D, int axis) {
    int npb, nkb, per, nslab;
    gru_wgrad_slabs(Cx, B, H, W, D, axis, npb, nkb, per, nslab);
    return (size_t)nslab * 3 * GG_HID * (GG_HID + Cx) * 5 * sizeof(float);
}

template <typename T, int NP>
__global__ __launch_bounds__(256, 1) void k_gru_wgrad(GruWgradArgs A) {
    constexpr int AROW = GW_P * GW_L * 2, BROW = (GW_P + 4) * GW_L * 2;   // 256, 512 bytes: 16, 32 slots of 16 bytes
    constexpr int APIECE = GG_HID * AROW, BPIECE = 16 * BROW;
    constexpr int AIT = GG_HID * GW_P * (GW_L / 2) / 256, BIT = 16 * (GW_P + 4) * (GW_L / 2) / 256;   // 24, 8 pairs
    __shared__ __attribute__((aligned(16))) unsigned char smem[NP * (APIECE + BPIECE)];
    static_assert(NP * (APIECE + BPIECE) >= 4 * 5 * 1024, "the epilogue's exchange buffer");
    unsigned char *as = smem, *bs = smem + NP * APIECE;
    const GruGeom &G = A.G;
    const int tid = threadIdx.x, lane = tid & 63, m16 = lane & 15, h4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned bid = blockIdx.x;
    const int slab = (int)(bid % (unsigned)A.nslab);
    bid /= (unsigned)A.nslab;
    const int gate = (int)(bid % 3u), cit = (int)(bid / 3u);
    const int cin = GG_HID + G.Cx, c0 = 16 * cit;
    const long long HWD = G.HWD;
    const float *a = gate == 0 ? A.az : gate == 1 ? A.ar : A.aq;
    const bool hid = c0 < GG_HID;        // a tile is all hidden or all input channels (96 = 6 x 16)
    const bool rh = hid && gate == 2;    // q's hidden columns: r h

    // staging: this thread's pair of lines (2 lp, 2 lp + 1); A: position apos, channels ao + 4 i; B: halo position bhp,
    // channels bci + 2 i
    const int lp = tid & 15, apos = (tid >> 4) & 3, ao = tid >> 6, bhp = (tid >> 4) & 7, bci = tid >> 7;
    float av[AIT][2], bv[BIT][2], rv[BIT][2];

    auto stage_load = [&](int kb) __attribute__((always_inline)) {
        const int lgrp = kb / A.npb, p0 = (kb - lgrp * A.npb) * GW_P;
        int b[2];
        long long off[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) ok[e] = gru_line(G, lgrp * GW_L + 2 * lp + e, b[e], off[e]);
        {
            const int pos = p0 + apos;
            const bool okp = pos < G.len;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float *p = a + (long long)b[e] * GG_HID * HWD + off[e] + (okp ? (long long)pos * G.pstride : 0);
#pragma unroll
                for (int i = 0; i < AIT; ++i) av[i][e] = ok[e] && okp ? p[(long long)(ao + 4 * i) * HWD] : 0.0f;
            }
        }
        const int pos = p0 - 2 + bhp;
        const bool okp = pos >= 0 && pos < G.len;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const long long voff = off[e] + (okp ? (long long)pos * G.pstride : 0);
#pragma unroll
            for (int i = 0; i < BIT; ++i) {
                const int c = c0 + bci + 2 * i;
                const bool okc = ok[e] && okp && c < cin;
                const long long hidx = ((long long)b[e] * GG_HID + (hid ? c : 0)) * HWD + voff;
                const long long xidx = ((long long)b[e] * G.Cx + (hid || !okc ? 0 : c - GG_HID)) * HWD + voff;
                bv[i][e] = okc ? (hid ? A.h[hidx] : A.x[xidx]) : 0.0f;
                rv[i][e] = okc && rh ? A.r[hidx] : 1.0f;
            }
        }
    };
    auto stage_write = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < AIT; ++i) {
            unsigned hi, lo;
            split2<T, NP>(av[i][0], av[i][1], hi, lo);
            const int o = ao + 4 * i;
            unsigned char *p = as + o * AROW + (((apos * 4 + (lp >> 2)) ^ (o & 15)) * 16) + (lp & 3) * 4;
            *reinterpret_cast<unsigned *>(p) = hi;
            if constexpr (NP == 2) *reinterpret_cast<unsigned *>(p + APIECE) = lo;
        }
#pragma unroll
        for (int i = 0; i < BIT; ++i) {
            unsigned hi, lo;
            split2<T, NP>(bv[i][0] * rv[i][0], bv[i][1] * rv[i][1], hi, lo);
            const int c = bci + 2 * i;
            unsigned char *p = bs + c * BROW + (((bhp * 4 + (lp >> 2)) ^ c) * 16) + (lp & 3) * 4;
            *reinterpret_cast<unsigned *>(p) = hi;
            if constexpr (NP == 2) *reinterpret_cast<unsigned *>(p + BPIECE) = lo;
        }
    };

    f32x4 acc[6][5];
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[t][k] = f32x4{0.f, 0.f, 0.f, 0.f};

    int kb = slab * A.per;
    const int kend = kb + A.per < A.nkb ? kb + A.per : A.nkb;
    stage_load(kb);
#pragma unroll 1
    for (; kb < kend; ++kb) {
        __syncthreads();   // the previous K-block's reads are done
        stage_write();
        __syncthreads();
        if (kb + 1 < kend) stage_load(kb + 1);
        // wave w: position w of the block; lane (m16, h4): row / column m16, lines 8 h4 .. 8 h4 + 7
        u32x4 af[6][NP];
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                af[t][pc] = *reinterpret_cast<const u32x4 *>(as + pc * APIECE + (16 * t + m16) * AROW +
                                                             (((wave * 4 + h4) ^ m16) * 16));
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            u32x4 bf[NP];
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                bf[pc] = *reinterpret_cast<const u32x4 *>(bs + pc * BPIECE + m16 * BROW +
                                                          ((((wave + k) * 4 + h4) ^ m16) * 16));
#pragma unroll
            for (int t = 0; t < 6; ++t) acc[t][k] = mma_step<T, NP>(af[t], bf, acc[t][k]);
        }
    }

    // the four waves' partial sums meet in LDS, one o tile (five taps) per round, summed in wave order.  Lane (m16, h4)
    // holds input channel c0 + m16, output channels 16 tile + 4 h4 + k.
    float *red = reinterpret_cast<float *>(smem);
    float *wsl = A.ws + ((long long)slab * 3 + gate) * GG_HID * cin * 5;
    const int rl = tid >> 2, rk = tid & 3;
    const int rci = c0 + (rl & 15);
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int ro = 16 * t + 4 * (rl >> 4) + rk;
        __syncthreads();   // the main loop's reads, or the previous round's, are done
#pragma unroll
        for (int k = 0; k < 5; ++k) *reinterpret_cast<f32x4 *>(red + ((wave * 5 + k) * 64 + lane) * 4) = acc[t][k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float s = ((red[k * 256 + tid] + red[1280 + k * 256 + tid]) + red[2560 + k * 256 + tid]) +
                            red[3840 + k * 256 + tid];
            if (rci < cin) wsl[((long long)ro * cin + rci) * 5 + k] = s;
        }
    }
}

// host entry: arguments validated by dvc_gru_wgrad (capi.hip)
hipError_t launch_gru_wgrad(const float *h, const float *x, const float *r, const float *az, const float *ar,
                            const float *aq, float *dw, void *workspace, int B, int Cx, int H, int W, int D, int axis,
                            int dtype, hipStream_t s) {
    GruWgradArgs A;
    A.G = gru_geom(B, Cx, H, W, D, axis);
    A.h = h; A.x = x; A.r = r; A.az = az; A.ar = ar; A.aq = aq; A.ws = static_cast<float *>(workspace);
    A.ncit = (GG_HID + Cx + 15) / 16;
    gru_wgrad_slabs(Cx, B, H, W, D, axis, A.npb, A.nkb, A.per, A.nslab);
    const unsigned grid = (unsigned)(A.nslab * 3 * A.ncit);
    with_precision(dtype, [&](auto t, auto np) {
        k_gru_wgrad<decltype(t), decltype(np)::value><<<grid, 256, 0, s>>>(A);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wgrad_reduce(A.ws, dw, 3 * GG_HID * (GG_HID + Cx) * 5, A.nslab, s);
}

}  // namespace dvc
