// fused_proj_f32.hip -- the fp32 on-the-fly lookup with the motion encoder's convc1 fused (round 7)
// (reference: CorrBlockOnTheFly in fp32, src/core/corr_otf.py:96-237, the evaluation path of legacy checkpoints,
// src/core/raft_dvc.py:403-412, followed by F.relu(self.convc1(corr)), src/core/update.py:219-222, 246).
//
// k_fused_proj (fused_proj.hip) for an fp32 block: the same origin-sorted chunks of 64 queries (k_otf_keys + radix
// sort, XCD-contiguous chunk order) and the same convc1 slicing (dvc_proj_pack's 3-column slices), with
//   phase 1  the window dots of k_fused_box_f32: packed fp32 queries and targets split in registers into three bf16
//            pieces, six v_mfma_f32_16x16x32_bf16 per step (split8 / mma6, fused_common.h), scaled by 1/sqrt(C)
//            and kept in fp32 -- the values CorrBlockFused(precision="fp32")(coords) interpolates;
//   phase 2  k_fused_box_f32's trilinear arithmetic; each output row goes to LDS as a bf16 hi tile and a lo tile
//            (x = xh + xl + O(2^-16 x)) and the consumers run k_lookup_tile<PROJ = 2>'s exact split convc1,
//            xh wh + xl wh + xh wl on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, over the hi block then the lo
//            block of dvc_proj_pack_exact;
//   output   relu(D + b) as one 384-byte row per query into the [B][Nq][96] workspace (k_rows_to_channels transposes).
//
// LDS.  fp32 windows are twice the bf16 kernel's bytes, so the (2r+2)^3 window goes through LDS in k_fused_box_f32's
// two passes of r+1 planes (2056 B per query at r = 4), the previous plane's z-lerps carried in registers across the
// pass boundary; the hi + lo X tiles (2 x 64 x 208 B at r = 4) sit beside the windows, 155.6 KB of the 160 KB with
// the 1 KB by which the parked z-lerps of the second pass (below) outgrow the X tiles.
//
// Waves.  The split query operands take 192 VGPRs at C_pad 128 (Split3 bq[4][4]), so the workgroup is four waves,
// one per SIMD (512 registers each), as k_fused_box_f32.  All four run phase 1; in phase 2 waves 0 .. NWV-1 produce
// three output columns each and every wave consumes: the six 16-channel output tiles are dealt 1, 1, 2, 2 to waves
// 0 .. 3 (the waves that produce least multiply most).
//
// Edge semantics are k_fused_proj's: inactive slots of the last chunk are never stored; dead (NaN / huge)
// coordinates and windows that miss a level have all-zero weights there and yield relu(bias); size-1 levels are
// skipped; the targets are read through an exactly sized buffer resource; no atomics.
#include "common.h"
#include "fused_common.h"
#include "lookup_common.h"

#include <type_traits>

namespace dvc {

template <int R> struct OtfProjF32Cfg {
    static constexpr int n = 2 * R + 1, NW = 2 * R + 2, NP = n / 2;
    static constexpr int PP = R + 1;                        // window planes per pass (NW = 2 PP)
    static constexpr int ROWB = NW * 4;                     // bytes of one window z-row (fp32, starts at the run)
    static constexpr int SLICE = PP * NW * ROWB;            // bytes of one query's window slice
    // query stride as BoxF32Cfg: 8-byte aligned and = 2 dwords mod 64 banks
    static constexpr int WQ = SLICE + 4 * ((2 - SLICE / 4) % 64 + 64) % 256;
    static constexpr int GUARD = 64;
    static constexpr int NWV = (n + 2) / 3;                 // producer waves, 3 output columns each (dvc_proj_pack)
    static constexpr int XROW = NWV * 64 + 16;              // bytes per query row of one X tile (+16: bank spread)
    static constexpr int XOFF = GUARD + 64 * WQ + GUARD;    // X hi tile; the lo tile 64 XROW after it
    // the X tiles are idle during phase 1: the second pass parks the producers' carried z-lerps there ([value][lane]
    // per producer wave), which takes them out of the registers live under the MFMA loop
    static constexpr int ZPW = 4 * n * 64 * 4;              // bytes per producer wave: (3 + 1) columns x n values x 64 lanes
    static constexpr int XBYTES = 2 * 64 * XROW > NWV * ZPW ? 2 * 64 * XROW : NWV * ZPW;
    static constexpr int LDS = (XOFF + XBYTES + 15) & ~15;
    static constexpr int NWAVES = 4;
    static constexpr int COUT = 96, OT = COUT / 16;
    static_assert((WQ / 4) % 64 == 2 && WQ % 8 == 0, "window stride");
    static_assert(XOFF % 16 == 0 && XROW % 16 == 0, "X tiles are read and written 16 bytes at a time");
    static_assert(NWV <= NWAVES, "not enough waves for the output columns");
    static_assert(3 * NP + 2 <= 16, "one wave's row values must fit a 32-k slice");
    static_assert(LDS <= 160 * 1024, "LDS");
};

template <int R, int KS>
__global__ __launch_bounds__(256, 1) void k_fused_proj_f32(const float *__restrict__ Q, const float *__restrict__ Tt,
                                                           LookupArgs A, const unsigned long long *__restrict__ keys,
                                                           int b, int Cp, long long t_rows, float scale,
                                                           float *__restrict__ rows_out) {
    using C = OtfProjF32Cfg<R>;
    constexpr int n = C::n, NW = C::NW, PP = C::PP, NP = C::NP, NWV = C::NWV, OT = C::OT, NWAVES = C::NWAVES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS];
    unsigned char *xs = smem + C::XOFF;   // X hi [64 q][XROW], then X lo
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long Nq = A.Nq;

    // XCD-aware chunk order (as k_fused_proj): each XCD a contiguous range of chunks
    const int nchunks = (int)((Nq + 63) / 64);
    const int per_xcd = (nchunks + 7) / 8;
    const int chunk = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (chunk >= nchunks) return;

    for (int i = tid * 16; i < C::LDS; i += 64 * NWAVES * 16)
        *reinterpret_cast<u32x4 *>(smem + i) = u32x4{0, 0, 0, 0};

    const long long slot = (long long)chunk * 64 + lane;
    const bool active = slot < Nq;
    const int q = active ? (int)(unsigned)(keys[slot] & 0xffffffffull) : 0;
    float cy = 0.f, cx = 0.f, cz = 0.f;
    if (active) load_coords(A.coords, b, Nq, q, cy, cx, cz);

    const int m16 = lane & 15, h4 = lane >> 4;
    int qrow[4];   // query of slot 16 j + m16 (inactive slots hold query 0: valid rows, never written)
#pragma unroll
    for (int j = 0; j < 4; ++j) qrow[j] = __shfl(q, 16 * j + m16);
    // packed fp32 targets of this batch element as a buffer (exact byte size, < 2^31 - 64 KB, checked on the host):
    // rows past a union's z range are addressed out of range and read as zeros
    const float *tb = Tt + (long long)b * t_rows * Cp;
    const unsigned long long tbp = (unsigned long long)tb;
    const unsigned tblo = __builtin_amdgcn_readfirstlane((unsigned)tbp);
    const unsigned tbhi = __builtin_amdgcn_readfirstlane((unsigned)(tbp >> 32));
    const int t_bytes = (int)(t_rows * Cp * 4);
    const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(((unsigned long long)tbhi << 32) | tblo), (short)0, t_bytes, 0x00020000);

    const int legacy = buni(A.legacy);
    const int u0 = wave * 3;                          // producer: output columns u0 .. u0 + NU - 1
    // consumer: output tiles 3 - wave and (waves 2, 3) 7 - wave, 16 channels each
    const int ntile = wave >= 2 ? 2 : 1;
    const int otile[2] = {3 - wave, wave >= 2 ? 7 - wave : 0};
    f32x4 acc[2][4];   // acc[t][j][i] = D[o = 16 otile[t] + 4 h4 + i][slot 16 j + m16]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the packed convc1 weights as a buffer: [level][row][slice ks][tile ot][lane] x 8 bf16, the hi block then the lo
    // block (dvc_proj_pack_exact), 1 KB per (row, slice, tile)
    const int wlo = buni(A.Ltot) * n * NWV * OT * 1024;   // bytes of one block
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
        buniptr(const_cast<void *>(A.proj_w)), (short)0, 2 * wlo, 0x00020000);
    __syncthreads();   // LDS cleared

    auto level = [&](int l, auto nu_c) {
        constexpr int NU = decltype(nu_c)::value;
        const int Hl = buni(A.H[l]), Wl = buni(A.W[l]), Dl = buni(A.D[l]), Dpl = buni(A.Dp[l]);
        const long long offl = buni64(A.off[l]);
        const float sc = (float)(1 << l);
        WinAxes ax;
        window_axes(cy / sc, cx / sc, cz / sc, Hl, Wl, Dl, legacy, ax);
        const int ih = (int)ax.kh - R, iu = (int)ax.ku - R, iv = (int)ax.kv - R;
        // a window that misses the level has all weights 0: it takes no part in the union
        const bool meets = ih < Hl && ih + NW > 0 && iu < Wl && iu + NW > 0 && iv < Dl && iv + NW > 0;
        const bool live = active && !ax.dead && meets;

        const int BIG = 1 << 29;
        const int ihmin = bwave_min(live ? ih : BIG), ihmax = bwave_max(live ? ih : -BIG);
        const int xs0 = max(bwave_min(live ? iu : BIG), 0), xe = min(bwave_max(live ? iu : -BIG) + NW - 1, Wl - 1);
        const int zs = max(bwave_min(live ? iv : BIG), 0), ze = min(bwave_max(live ? iv : -BIG) + NW - 1, Dl - 1);
        const int nx = xe - xs0 + 1, nz = ze - zs + 1;
        const int nzb = (nz + 15) / 16;

        // per B block j: value (y, x, z) of the window slice of pass p of slot 16 j + m16 lands at
        //   GUARD + slot * WQ + ((y - ih - P0) * NW + (x - iu)) * ROWB + (z - iv) * 4
        // = wb[j] - P0 * NW * ROWB + (y * NW + x) * ROWB + z * 4
        int oh[4], ou[4], ov[4], wb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int src = 16 * j + m16;
            const int sh = __shfl(ih, src);
            oh[j] = __shfl((int)live, src) ? sh : -BIG;     // dead / inactive / missing windows take no values
            ou[j] = __shfl(iu, src);
            ov[j] = __shfl(iv, src);
            wb[j] = C::GUARD + src * C::WQ - (sh * NW + ou[j]) * C::ROWB - ov[j] * 4;
        }

        BRun<n> zp[NU + 1];   // z-lerps of the current row's lower plane (carried across the two passes)

        auto pass = [&](auto p_c) {
            constexpr int P = decltype(p_c)::value;
            constexpr int P0 = P * PP;   // first window plane of the slice
            __syncthreads();             // the previous slice's phase-2 reads are done (windows and X)
            [[maybe_unused]] float *zst = reinterpret_cast<float *>(xs + wave * C::ZPW) + lane;
            if constexpr (NU > 0 && P == 1) {   // park the carried z-lerps in the idle X region
#pragma unroll
                for (int k = 0; k <= NU; ++k) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        zst[((k * n) + 2 * i) * 64] = zp[k].p[i][0];
                        zst[((k * n) + 2 * i + 1) * 64] = zp[k].p[i][1];
                    }
                    zst[((k * n) + n - 1) * 64] = zp[k].t;
                }
            }
            // ---------------- phase 1: the slice's window dots on MFMA (k_fused_box_f32's loop) ----------------
            const int ys = max(ihmin + P0, 0), ye = min(ihmax + P0 + PP - 1, Hl - 1);
            const int ny = ye - ys + 1;
            if (ny > 0 && nx > 0 && nz > 0) {
                // MFMA B operands (the chunk's queries as three bf16 pieces), reloaded and split per pass (L2 hits) so
                // that their 48 KS registers are free in phase 2: block j = slots 16 j .. 16 j + 15, lane i holds the
                // query of slot 16 j + (i & 15), channels 32 ks + 8 (i >> 4) .. + 7
                Split3 bq[4][KS];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float *row = Q + ((long long)b * Nq + qrow[j]) * Cp;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const f32x4 lo4 = *reinterpret_cast<const f32x4 *>(row + 32 * ks + 8 * h4);
                        const f32x4 hi4 = *reinterpret_cast<const f32x4 *>(row + 32 * ks + 8 * h4 + 4);
                        bq[j][ks] = split8(lo4, hi4);
                    }
                }
                const int nrows = ny * nx;
                const int nit = nrows > wave ? (nrows - wave + NWAVES - 1) / NWAVES * nzb : 0;
                struct Pos { int by, bx, zb; };
                auto advance = [&](Pos &ps) {
                    if (++ps.zb < nzb) return;
                    ps.zb = 0;
                    ps.bx += NWAVES;
                    while (ps.bx >= nx) { ps.bx -= nx; ps.by += 1; }
                };
                Pos pl;
                pl.zb = 0;
                pl.by = wave / nx;
                pl.bx = wave - pl.by * nx;
                Pos pe = pl;
                int nload = 0;
                // raw fp32 target rows, two 16-byte pieces per channel step; unconditional loads (out of range,
                // zeros, past the wave's last block) keep the waitcnt bookkeeping exact, as in k_fused_box
                auto load_a = [&](f32x4 (&dst)[KS][2]) {
                    const int z0 = zs + 16 * pl.zb;
                    const long long rowbase = offl + ((long long)(ys + pl.by) * Wl + (xs0 + pl.bx)) * Dpl;
                    const int off = nload < nit && z0 + m16 <= ze ? (int)(((rowbase + z0 + m16) * Cp + 8 * h4) * 4)
                                                                  : 0x7fff0000;
                    ++nload;
                    advance(pl);
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        dst[ks][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_t, off + 128 * ks, 0, 0));
                        dst[ks][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_t, off + 128 * ks + 16, 0, 0));
                    }
                };
                auto mfma = [&](const f32x4 (&a)[KS][2], f32x4 (&d)[4]) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const Split3 as = split8(a[ks][0], a[ks][1]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) d[j] = mma6(as, bq[j][ks], d[j]);
                    }
                };
                int rowok = 0;   // bit j: the row is inside the window slice of slot 16 j + m16
                auto epilogue = [&](const f32x4 (&d)[4]) {
                    const int z0 = zs + 16 * pe.zb;
                    const int y = ys + pe.by, x = xs0 + pe.bx;
                    if (pe.zb == 0) {
                        rowok = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            rowok |= (int)((unsigned)(y - oh[j] - P0) < (unsigned)PP &&
                                           (unsigned)(x - ou[j]) < (unsigned)NW) << j;
                    }
                    advance(pe);
                    const int rowu = (y * NW + x) * C::ROWB - P0 * NW * C::ROWB;
                    const int zl = z0 + 4 * h4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int base = wb[j] + rowu + zl * 4;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const bool in = ((rowok >> j) & 1) && (unsigned)(zl + i - ov[j]) < (unsigned)NW;
                            if (in) *reinterpret_cast<float *>(smem + base + 4 * i) = d[j][i] * scale;   // (masked)
                        }
                    }
                };
                f32x4 a0[KS][2], a1[KS][2];
                f32x4 c0[4], c1[4];
                if (nit > 0) {
                    load_a(a0);
                    load_a(a1);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma(a0, c0);
                    load_a(a0);
                    for (int k = 0; k < nit; k += 2) {
                        mfma(a1, c1);
                        load_a(a1);
                        epilogue(c0);
                        mfma(a0, c0);
                        load_a(a0);
                        if (k + 1 < nit) epilogue(c1);
                    }
                }
            }
            __syncthreads();   // the slice's windows complete
            // ---------------- phase 2: the rows whose upper plane is in the slice -> X tiles -> convc1 ----------------
            // phase-2 weights of this lane's query (the producers' only; computed per pass: not live under phase 1)
            float wv0[n], wv1[n];
            f32x2 w0p[NP], w1p[NP];
            if constexpr (NU > 0) {
    #pragma unroll
                for (int tt = 0; tt < n; ++tt) {
                    axis_weights(ax.pv, ax.kv, tt - R, ax.vn, ax.vu, wv0[tt], wv1[tt]);
                    wv0[tt] = (unsigned)(iv + tt) < (unsigned)Dl ? wv0[tt] : 0.0f;
                    wv1[tt] = (unsigned)(iv + tt + 1) < (unsigned)Dl ? wv1[tt] : 0.0f;
                }
    #pragma unroll
                for (int i = 0; i < NP; ++i) {
                    w0p[i] = f32x2{wv0[2 * i], wv0[2 * i + 1]};
                    w1p[i] = f32x2{wv1[2 * i], wv1[2 * i + 1]};
                }
            }
            float wx0[NU > 0 ? NU : 1], wx1[NU > 0 ? NU : 1];
    #pragma unroll
            for (int uu = 0; uu < NU; ++uu) {
                const int u = u0 + uu;
                axis_weights(ax.pu, ax.ku, u - R, ax.un, ax.uu, wx0[uu], wx1[uu]);
                wx0[uu] = (unsigned)(iu + u) < (unsigned)Wl ? wx0[uu] : 0.0f;
                wx1[uu] = (unsigned)(iu + u + 1) < (unsigned)Wl ? wx1[uu] : 0.0f;
            }
            const unsigned char *myw = smem + C::GUARD + lane * C::WQ;
            auto lerp_col = [&](int wpl, int k, BRun<n> &z) {   // window plane wpl of the current slice, column u0 + k
                const f32x2 *p = reinterpret_cast<const f32x2 *>(myw + (wpl * NW + u0 + k) * C::ROWB);
                float r[NW];
    #pragma unroll
                for (int i = 0; i < NW / 2; ++i) {
                    const f32x2 d = p[i];
                    r[2 * i] = d[0];
                    r[2 * i + 1] = d[1];
                }
    #pragma unroll
                for (int i = 0; i < NP; ++i)
                    z.p[i] = __builtin_elementwise_fma(f32x2{r[2 * i + 1], r[2 * i + 2]}, w1p[i],
                                                       f32x2{r[2 * i], r[2 * i + 1]} * w0p[i]);
                z.t = __builtin_fmaf(r[n], wv1[n - 1], r[n - 1] * wv0[n - 1]);
            };
            if constexpr (NU > 0 && P == 0) {
#pragma unroll
                for (int k = 0; k <= NU; ++k) lerp_col(0, k, zp[k]);
            }
            if constexpr (NU > 0 && P == 1) {   // (the first X write of this pass comes after the next barrier)
#pragma unroll
                for (int k = 0; k <= NU; ++k) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        zp[k].p[i] = f32x2{zst[((k * n) + 2 * i) * 64], zst[((k * n) + 2 * i + 1) * 64]};
                    zp[k].t = zst[((k * n) + n - 1) * 64];
                }
            }
            constexpr int A0 = P == 0 ? 0 : PP - 1, A1 = P == 0 ? PP - 1 : n;   // rows [A0, A1)
            for (int a = A0; a < A1; ++a) {
                // this row's weights of the wave's tiles: [slice ks][tile ot][lane] x 8 bf16, hi block then lo block
                bf16x8 wh[2][NWV], wl[2][NWV];
                const int wr = (l * n + a) * NWV * OT * 1024;
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (t < ntile) {
#pragma unroll
                        for (int ks = 0; ks < NWV; ++ks) {
                            const int wo = wr + (ks * OT + otile[t]) * 1024;
                            wh[t][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, wo, 0));
                            wl[t][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, wlo + wo, 0));
                        }
                    }
                unsigned xw[16], xwl[16];   // producer: this wave's 32-k slice of row a as bf16 pairs, hi and lo
                if constexpr (NU > 0) {
                    float wy0, wy1;
                    axis_weights(ax.ph, ax.kh, a - R, ax.hs, ax.hs, wy0, wy1);
                    wy0 = (unsigned)(ih + a) < (unsigned)Hl ? wy0 : 0.0f;
                    wy1 = (unsigned)(ih + a + 1) < (unsigned)Hl ? wy1 : 0.0f;
                    BRun<n> zc[NU + 1];
#pragma unroll
                    for (int k = 0; k <= NU; ++k) lerp_col(a + 1 - P0, k, zc[k]);
                    unsigned xr[NU * NP], xrl[NU * NP];
                    float xt[NU];
#pragma unroll
                    for (int uu = 0; uu < NU; ++uu) {
                        const float p00 = wx0[uu] * wy0, p10 = wx1[uu] * wy0;
                        const float p01 = wx0[uu] * wy1, p11 = wx1[uu] * wy1;
                        // broadcasts materialised (splat2): other waves run MFMAs meanwhile
                        const f32x2 P00 = splat2(p00), P10 = splat2(p10), P01 = splat2(p01), P11 = splat2(p11);
#pragma unroll
                        for (int i = 0; i < NP; ++i) {
                            f32x2 v = P00 * zp[uu].p[i];
                            v = __builtin_elementwise_fma(P10, zp[uu + 1].p[i], v);
                            v = __builtin_elementwise_fma(P01, zc[uu].p[i], v);
                            v = __builtin_elementwise_fma(P11, zc[uu + 1].p[i], v);
                            const bf16x2 hv = __builtin_convertvector(v, bf16x2);
                            xr[uu * NP + i] = __builtin_bit_cast(unsigned, hv);
                            xrl[uu * NP + i] = __builtin_bit_cast(
                                unsigned, __builtin_convertvector(v - __builtin_convertvector(hv, f32x2), bf16x2));
                        }
                        float v = p00 * zp[uu].t;
                        v = __builtin_fmaf(p10, zp[uu + 1].t, v);
                        v = __builtin_fmaf(p01, zc[uu].t, v);
                        v = __builtin_fmaf(p11, zc[uu + 1].t, v);
                        xt[uu] = v;
                    }
#pragma unroll
                    for (int k = 0; k <= NU; ++k) zp[k] = zc[k];
                    // slice order (dvc_proj_pack): pairs (column uu, v = 2i, 2i + 1), then the tails, then zeros
                    constexpr int T0 = NU * NP;
#pragma unroll
                    for (int d = 0; d < 16; ++d) {
                        xw[d] = d < T0 ? xr[d < T0 ? d : 0] : 0u;
                        xwl[d] = d < T0 ? xrl[d < T0 ? d : 0] : 0u;
                    }
#pragma unroll
                    for (int p = 0; 2 * p < NU; ++p) {
                        const f32x2 t2 = {xt[2 * p], 2 * p + 1 < NU ? xt[2 * p + 1 < NU ? 2 * p + 1 : 0] : 0.0f};
                        const bf16x2 hv = __builtin_convertvector(t2, bf16x2);
                        xw[T0 + p] = __builtin_bit_cast(unsigned, hv);
                        xwl[T0 + p] = __builtin_bit_cast(
                            unsigned, __builtin_convertvector(t2 - __builtin_convertvector(hv, f32x2), bf16x2));
                    }
                }
                __syncthreads();   // every wave has read row a - 1 of X
                if constexpr (NU > 0) {
                    u32x4 *dh = reinterpret_cast<u32x4 *>(xs + lane * C::XROW + wave * 64);
                    u32x4 *dl = reinterpret_cast<u32x4 *>(xs + (64 + lane) * C::XROW + wave * 64);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        dh[j] = u32x4{xw[4 * j], xw[4 * j + 1], xw[4 * j + 2], xw[4 * j + 3]};
                        dl[j] = u32x4{xwl[4 * j], xwl[4 * j + 1], xwl[4 * j + 2], xwl[4 * j + 3]};
                    }
                }
                __syncthreads();   // row a complete in X
#pragma unroll
                for (int ks = 0; ks < NWV; ++ks) {
                    bf16x8 xh[4], xl[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int xo = (16 * j + m16) * C::XROW + ks * 64 + h4 * 16;
                        xh[j] = *reinterpret_cast<const bf16x8 *>(xs + xo);
                        xl[j] = *reinterpret_cast<const bf16x8 *>(xs + 64 * C::XROW + xo);
                    }
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        if (t < ntile) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[t][ks], xh[j], acc[t][j], 0, 0, 0);
                                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[t][ks], xl[j], acc[t][j], 0, 0, 0);
                                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[t][ks], xh[j], acc[t][j], 0, 0, 0);
                            }
                        }
                }
            }
        };
        pass(std::integral_constant<int, 0>{});
        pass(std::integral_constant<int, 1>{});
    };

    constexpr int NU_LAST = n - 3 * (NWV - 1);
    for (int l = 0; l < A.Ltot; ++l) {
        if (buni(A.zero[l])) continue;   // a size-1 level samples zeros: nothing reaches convc1
        if (wave < NWV - 1) level(l, std::integral_constant<int, 3>{});
        else if (wave == NWV - 1) level(l, std::integral_constant<int, NU_LAST>{});
        else level(l, std::integral_constant<int, 0>{});
    }

    // relu(D + b) -> rows_out[b][q][96]: lane (m16, h4) stores channels 16 ot + 4 h4 .. + 3 of the query of slot
    // 16 j + m16 (16 queries x 64 contiguous bytes per wave store)
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (t < ntile) {
            const int o0 = 16 * otile[t] + 4 * h4;
            const f32x4 bias = {A.proj_b[o0], A.proj_b[o0 + 1], A.proj_b[o0 + 2], A.proj_b[o0 + 3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ok = __shfl((int)active, 16 * j + m16);
                f32x4 v = acc[t][j] + bias;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] < 0.f ? 0.f : v[i];   // relu (NaN kept)
                if (ok) *reinterpret_cast<f32x4 *>(rows_out + ((long long)b * Nq + qrow[j]) * C::COUT + o0) = v;
            }
        }
}

// r = 1 and r = 2 instances live in fused_proj_f32_r12.hip, compiled without SLP vectorisation: with it each of them
// gets one SLP-formed packed-FP32 add whose low lane reads the high half of a pair (the hazard tools/isa_check.py
// guards, see splat2 in common.h); r = 3 and r = 4 compile clean with SLP.
#define DVC_FPROJ_F32_R12(R, KS)                                                                                   \
    extern template __global__ void k_fused_proj_f32<R, KS>(const float *, const float *, LookupArgs,               \
                                                            const unsigned long long *, int, int, long long, float, \
                                                            float *);
#ifndef DVC_FPROJ_F32_R12_TU
DVC_FPROJ_F32_R12(1, 1) DVC_FPROJ_F32_R12(1, 2) DVC_FPROJ_F32_R12(1, 4)
DVC_FPROJ_F32_R12(2, 1) DVC_FPROJ_F32_R12(2, 2) DVC_FPROJ_F32_R12(2, 4)
#endif
#undef DVC_FPROJ_F32_R12

#ifndef DVC_FPROJ_F32_R12_TU
template <int R>
static void launch_proj_f32_r(const float *Q, const float *Tt, const LookupArgs &A, const unsigned long long *keys,
                              int b, int Cp, long long t_rows, float scale, float *rows, hipStream_t s) {
    const long long nchunks = (A.Nq + 63) / 64;
    const unsigned grid = (unsigned)(8 * ((nchunks + 7) / 8));
    switch (Cp / 32) {
    case 1: k_fused_proj_f32<R, 1><<<grid, 256, 0, s>>>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows); break;
    case 2: k_fused_proj_f32<R, 2><<<grid, 256, 0, s>>>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows); break;
    default: k_fused_proj_f32<R, 4><<<grid, 256, 0, s>>>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows); break;
    }
}

// host entry (fused_proj.hip): radius 1..4, C_pad in {32, 64, 128}, 32-bit target offsets, sorted keys of batch
// element b
void launch_fused_proj_f32(int radius, const float *Q, const float *Tt, const LookupArgs &A,
                           const unsigned long long *keys, int b, int Cp, long long t_rows, float scale, float *rows,
                           hipStream_t s) {
    switch (radius) {
    case 1: launch_proj_f32_r<1>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows, s); break;
    case 2: launch_proj_f32_r<2>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows, s); break;
    case 3: launch_proj_f32_r<3>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows, s); break;
    default: launch_proj_f32_r<4>(Q, Tt, A, keys, b, Cp, t_rows, scale, rows, s); break;
    }
}
#endif  // DVC_FPROJ_F32_R12_TU

}  // namespace dvc
