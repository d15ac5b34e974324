// lookup_coarse.h -- the coarse-level path of k_lookup_tile (lookup_tile.h): a level small enough that the rows of a
// whole 64-query tile fit LDS is staged whole, without the window table and the plane ring.
//
// For r = 4 the (2r+2)^3 window covers an 8^3 or 4^3 level entirely, and a unit of such a level writes 187 KB while it
// reads at most 64 KB; the plane pipeline (coordinates -> window table -> plane 0 -> plane 1 -> one barrier per row)
// only adds dependent round trips and barriers to it.  The level's part of a pyramid row is one contiguous segment
// (off[l], H_l W_l Dp_l elements) whose address does not depend on the coordinates, so
//   * the 64 segments are fetched with coalesced 16-byte loads issued back to back with the coordinate loads (one
//     memory round trip), through the tile's bounded buffer descriptor: rows past a ragged tile's end read zeros;
//   * they are written to LDS at GUARD + query * (segment bytes + 8): one barrier, after which the waves never meet
//     again -- each owns output columns, as in the tile kernel, and runs free;
//   * compute is the tile kernel's, operation for operation (window_axes / axis_weights float32 arithmetic, zero
//     padding folded into the weights, lds_run / lds_run_perm conversions, z-lerp, then the four (y, x) terms with
//     packed-f32 ops), so the outputs agree bit for bit.  A plane, column or z-run outside the level is clamped to an
//     address inside the staged image (or its zeroed pad / guards): it has weight 0 and only has to be finite.
// Included by lookup_tile.h (after lds_run, ZRun); the host's eligibility rule is coarse_level_ok (lookup_common.h).
#pragma once

namespace dvc {

// Levels [lc0, lc1) of the tile (b, qt), output rows [a0, a1), this wave's output columns u0 .. u0 + NU - 1.
// stamp / done: the caller's timeline hooks (diagnostics instances; no-ops otherwise).
template <typename T, int R, bool NT, int ABL, int SPOL, int NU, int THREADS, typename Stamp, typename Done>
__device__ __forceinline__ void coarse_unit(const LookupArgs &A, unsigned char *smem, int lc0, int lc1, int u0, int a0,
                                            int a1, int b, long long qt, int nvalid, Stamp &&stamp, Done &&done) {
    constexpr int n = 2 * R + 1, NW = 2 * R + 2, ES = (int)sizeof(T), NP = n / 2;
    constexpr long long n3 = (long long)n * n * n;
    constexpr int GUARD = kCoarseGuard, PAD = kCoarsePad;
    constexpr int KB = 16;   // 16-byte chunks in flight per thread (64 VGPRs): a 64 KB image in one batch of 256 threads
    constexpr int OOB = 0x7fff0000;
    static_assert(GUARD >= NW * ES + 4, "a clamped run may start NW elements before / end NW + 2 past the image");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const long long Nq = A.Nq;
    const long long q = A.q0 + qt + lane;
    const bool active = lane < nvalid;

    // the tile's rows as one buffer (as in k_lookup_tile): offsets past its valid rows read 0
    const T *tile_rows = reinterpret_cast<const T *>(A.corr) + ((long long)b * Nq + A.q0 + qt) * A.row_stride;
    const unsigned long long trp = (unsigned long long)tile_rows;
    const unsigned trlo = __builtin_amdgcn_readfirstlane((unsigned)trp);
    const unsigned trhi = __builtin_amdgcn_readfirstlane((unsigned)(trp >> 32));
    const int nrec = __builtin_amdgcn_readfirstlane((int)((long long)nvalid * A.row_stride * ES));
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(((unsigned long long)trhi << 32) | trlo), (short)0, nrec, 0x00020000);
    const int rs_b = (int)A.row_stride * ES;
    // output lane offset; lanes past the tile's end store out of the descriptor's range (dropped)
    const int q4 = active ? (int)(q * 4) : 0x7ffffff0;
    const int chstep_u = A.legacy ? 1 : n;
    const int chstep_v = A.legacy ? n : 1;
    auto out_rsrc = [&](float *obase, int a, int u) {
        return __builtin_amdgcn_make_buffer_rsrc(obase + ((long long)a * n * n + (long long)u * chstep_u) * Nq,
                                                 (short)0, (int)(n * n * Nq * 4), 0x00020000);
    };
    auto store = [&](__amdgpu_buffer_rsrc_t rs, int v, float val) {
        if constexpr ((ABL & 1) != 0) asm volatile("" ::"v"(val));
        else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), rs, q4, (int)(v * chstep_v * Nq * 4),
                                                   SPOL >= 0 ? SPOL : (NT ? 2 : 0));
    };

    // the coordinates and, right behind them, the first level's rows: one round trip
    float cy = 0.f, cx = 0.f, cz = 0.f;
    if (active) load_coords(A.coords, b, Nq, q, cy, cx, cz);

    for (int l = lc0; l < lc1; ++l) {
        const int Hl = A.H[l], Wl = A.W[l], Dl = A.D[l], Dpl = A.Dp[l];
        const int img_b = Hl * Wl * Dpl * ES;   // bytes of the level in one row: a multiple of 16 (Dp % 8 == 0)
        const int SQ = img_b + PAD;             // LDS bytes per query (+8: bank spread)
        const int cpq = img_b >> 4;             // 16-byte chunks per query
        const int nch = 64 * cpq;
        const int lev_b = (int)A.off[l] * ES;
        const float inv_cpq = 1.0f / (float)cpq;
        if (l > lc0) __syncthreads();           // the previous level's LDS reads are done

        // chunk idx -> (query j, chunk c of its segment): a float quotient, corrected to the exact one
        u32x4 st[KB];
        int lo[KB];   // LDS byte offset of the chunk (-1: none)
        auto issue = [&](int base) {
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const int idx = base + tid + k * THREADS;
                int j = (int)((float)idx * inv_cpq);
                int c = idx - j * cpq;
                if (c < 0) { --j; c += cpq; }
                else if (c >= cpq) { ++j; c -= cpq; }
                const bool ok = idx < nch;
                lo[k] = ok ? GUARD + j * SQ + c * 16 : -1;
                st[k] = __builtin_bit_cast(
                    u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, ok ? j * rs_b + lev_b + c * 16 : OOB, 0, 0));
            }
        };
        auto commit = [&]() {
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (lo[k] >= 0) {
                    *reinterpret_cast<u32x2 *>(smem + lo[k]) = u32x2{st[k][0], st[k][1]};
                    *reinterpret_cast<u32x2 *>(smem + lo[k] + 8) = u32x2{st[k][2], st[k][3]};
                }
        };
        issue(0);
        // pads and guards are read with weight 0 and must be finite
        if (tid < 64) *reinterpret_cast<u32x2 *>(smem + GUARD + tid * SQ + img_b) = u32x2{0, 0};
        if (tid < GUARD / 8) {
            *reinterpret_cast<u32x2 *>(smem + tid * 8) = u32x2{0, 0};
            *reinterpret_cast<u32x2 *>(smem + GUARD + 64 * SQ + tid * 8) = u32x2{0, 0};
        }

        // this lane's window and per-axis weights (reference float32 arithmetic), zero padding folded in
        float *obase = A.out + ((long long)b * A.Ltot + l) * n3 * Nq;   // wave-uniform
        const float sc = (float)(1 << l);
        WinAxes ax;
        window_axes(cy / sc, cx / sc, cz / sc, Hl, Wl, Dl, A.legacy, ax);
        const int ih = (int)ax.kh - R, iu = (int)ax.ku - R, iv = (int)ax.kv - R;
        float wv0[n], wv1[n];
#pragma unroll
        for (int t = 0; t < n; ++t) {
            axis_weights(ax.pv, ax.kv, t - R, ax.vn, ax.vu, wv0[t], wv1[t]);
            wv0[t] = (unsigned)(iv + t) < (unsigned)Dl ? wv0[t] : 0.0f;
            wv1[t] = (unsigned)(iv + t + 1) < (unsigned)Dl ? wv1[t] : 0.0f;
        }
        f32x2 w0p[NP], w1p[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            w0p[i] = f32x2{wv0[2 * i], wv0[2 * i + 1]};
            w1p[i] = f32x2{wv1[2 * i], wv1[2 * i + 1]};
        }
        float wx0[NU], wx1[NU];
#pragma unroll
        for (int uu = 0; uu < NU; ++uu) {
            const int u = u0 + uu;
            axis_weights(ax.pu, ax.ku, u - R, ax.un, ax.uu, wx0[uu], wx1[uu]);
            wx0[uu] = (unsigned)(iu + u) < (unsigned)Wl ? wx0[uu] : 0.0f;
            wx1[uu] = (unsigned)(iu + u + 1) < (unsigned)Wl ? wx1[uu] : 0.0f;
        }
        // LDS byte address of this lane's run in plane 0 of window column k; a run outside the level in z starts at
        // most NW elements before / at the end of its column: it stays inside the image, its pad or the guards
        const int rz = min(max(iv, -NW), Dpl);
        const int plane_b = Wl * Dpl * ES;
        int coff[NU + 1];
#pragma unroll
        for (int k = 0; k <= NU; ++k) {
            const int xc = min(max(iu + u0 + k, 0), Wl - 1);
            coff[k] = GUARD + lane * SQ + (xc * Dpl + rz) * ES;
        }
        constexpr bool BF = std::is_same<T, bf16_t>::value;
        unsigned sel_e = 0, sel_o = 0;   // bf16: v_perm selectors of the run parity (SQ, plane_b, Dpl * ES: multiples of 4)
        if constexpr (BF) bf16_run_selectors((rz & 1) != 0, sel_e, sel_o);
        auto lerp_col = [&](int y, int k, ZRun<n> &z) {
            const int addr = coff[k] + min(max(y, 0), Hl - 1) * plane_b;
            float r[NW];
            if constexpr (BF) lds_run_perm<NW>(smem, addr, sel_e, sel_o, r);
            else lds_run<NW>(smem, addr, (const T *)nullptr, r);
#pragma unroll
            for (int i = 0; i < NP; ++i)
                z.p[i] = __builtin_elementwise_fma(f32x2{r[2 * i + 1], r[2 * i + 2]}, w1p[i],
                                                   f32x2{r[2 * i], r[2 * i + 1]} * w0p[i]);
            z.t = __builtin_fmaf(r[n], wv1[n - 1], r[n - 1] * wv0[n - 1]);
        };
        stamp(1);

        commit();
        for (int base = THREADS * KB; base < nch; base += THREADS * KB) {
            issue(base);
            commit();
        }
        stamp(3);
        __syncthreads();   // the level is staged: the only meeting of the waves
        stamp(4);

        ZRun<n> zp[NU + 1];   // z-lerped columns of the lower plane of the current row
#pragma unroll
        for (int k = 0; k <= NU; ++k) lerp_col(ih + a0, k, zp[k]);
        stamp(5);
        for (int a = a0; a < a1; ++a) {
            float wy0, wy1;
            axis_weights(ax.ph, ax.kh, a - R, ax.hs, ax.hs, wy0, wy1);
            wy0 = (unsigned)(ih + a) < (unsigned)Hl ? wy0 : 0.0f;
            wy1 = (unsigned)(ih + a + 1) < (unsigned)Hl ? wy1 : 0.0f;
            ZRun<n> zprev;
#pragma unroll
            for (int k = 0; k <= NU; ++k) {
                ZRun<n> zcur;
                lerp_col(ih + a + 1, k, zcur);
                if (k >= 1) {
                    const int uu = k - 1;
                    const float p00 = wx0[uu] * wy0, p10 = wx1[uu] * wy0;
                    const float p01 = wx0[uu] * wy1, p11 = wx1[uu] * wy1;
                    const f32x2 P00 = {p00, p00}, P10 = {p10, p10}, P01 = {p01, p01}, P11 = {p11, p11};
                    const __amdgpu_buffer_rsrc_t rs = out_rsrc(obase, a, u0 + uu);
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        f32x2 acc = P00 * zp[uu].p[i];
                        acc = __builtin_elementwise_fma(P10, zp[uu + 1].p[i], acc);
                        acc = __builtin_elementwise_fma(P01, zprev.p[i], acc);
                        acc = __builtin_elementwise_fma(P11, zcur.p[i], acc);
                        store(rs, 2 * i, acc[0]);
                        store(rs, 2 * i + 1, acc[1]);
                    }
                    float acc = p00 * zp[uu].t;
                    acc = __builtin_fmaf(p10, zp[uu + 1].t, acc);
                    acc = __builtin_fmaf(p01, zprev.t, acc);
                    acc = __builtin_fmaf(p11, zcur.t, acc);
                    store(rs, n - 1, acc);
                    zp[uu] = zprev;
                }
                zprev = zcur;
                if (k == NU) zp[k] = zcur;
            }
            if (6 + a - a0 < 15) stamp(6 + a - a0);   // (15 is the caller's end stamp)
        }
        done();
    }
}

}  // namespace dvc
