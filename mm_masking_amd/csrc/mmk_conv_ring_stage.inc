// One stage of conv3x3_ring_kernel (mmk_unet.hip), included once per ring slot with STAGE_SLOT
// defined to the slot index: keeping the slot a literal keeps the register ring in VGPRs.
//
// Everything that touches global memory in here is straight-line code (no load, store or use of a
// loaded value sits under a branch): hipcc's s_waitcnt bookkeeping merges branches conservatively,
// and one uncertain count turns the wait for tile k+1 into a wait for every load in flight.
{
    const int k = k0 + STAGE_SLOT;
#if STAGE_CHECKED
    if (k >= nt_blk) goto ring_done;     // (first round and tail only; a skipped stage must not fall through to the next one)
#endif
    {
        constexpr int SN = (STAGE_SLOT + 1) % RD;                // slot of tile k+1
        const int pix0 = cur_pix0, ty0 = cur_ty0, tx0 = cur_tx0; // tile k (in LDS)
        MMK_STAMP(0);
        lds_barrier();      // tile k is in LDS; everyone is done reading tile k-1
        MMK_STAMP(1);
        // ---- operands of this tile's epilogue, ahead of everything else in the load queue
        bf16x4 e_src[EPI ? MT : 1][EPI ? NT : 1], e_acc[EPI ? MT : 1][EPI ? NT : 1];
        u32x4 e8_src = {0u, 0u, 0u, 0u}, e8_acc = {0u, 0u, 0u, 0u};
        if constexpr (EPI && C8) {
            const bool ok8 = (ty0 + lrow8) < a.H && (tx0 + lcol8) < a.W;
            const int off8 = (pix0 + lpix8) * 8;
            const u32x4 *ps = (ok8 && c8_has_src) ? reinterpret_cast<const u32x4 *>(a.o1.relu_src + off8) : &g_zero16;
            const u32x4 *pa = (ok8 && c8_accm) ? reinterpret_cast<const u32x4 *>(a.o1.y + off8) : &g_zero16;
            e8_src = *ps;
            e8_acc = *pa;
        }
        if constexpr (EPI && !C8) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const bool okp = (ty0 + 2 * wv + (n >> 1)) < a.H && (tx0 + (n & 1) * 16 + (lane & 15)) < a.W;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const bool ok = okp && o_cv[m];
                    const int off = pix0 * o_C[m] + o_loff[m][n];
                    const bf16x4 *ps = (ok && o_has_src[m]) ? reinterpret_cast<const bf16x4 *>(o_sb[m] + off)
                                                            : reinterpret_cast<const bf16x4 *>(&g_zero16);
                    const bf16x4 *pa = (ok && o_accm[m]) ? reinterpret_cast<const bf16x4 *>(o_yb[m] + off)
                                                         : reinterpret_cast<const bf16x4 *>(&g_zero16);
                    e_src[m][n] = *ps;
                    e_acc[m][n] = *pa;
                }
            }
        }
        // ---- stage tile k+1 into the other LDS buffer, re-arm its slot with tile k+1+RD
        // (unconditional: past the block's last tile the slot holds a duplicate of the last tile,
        // written to the LDS buffer nobody reads any more)
        const int pp0 = cur_pp0;
        cur_pix0 = s_pix0[SN]; cur_ty0 = s_ty0[SN]; cur_tx0 = s_tx0[SN];
        if constexpr (POOL) cur_pp0 = s_pp0[SN];
        MMK_RING_STORE(SN, (k + 1) & 1);
        MMK_STAMP(2);
        MMK_RING_LOAD(SN);
        MMK_STAMP(3);
        // ---- MFMA over the tile in LDS
        const bf16 *cur = in_tile + (k & 1) * (HT * WT * PK);
        f32x4 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
            const bf16 *bl = cur + b_lane[ks];
            bf16x8 bf[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n)
                bf[n] = *reinterpret_cast<const bf16x8 *>(bl + ((n >> 1) * WT + (n & 1) * 16) * PK);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const bf16x8 af = *reinterpret_cast<const bf16x8 *>(w_lds + ((size_t)((ks * MT + m) * 64 + lane)) * 8);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[n], acc[m][n], 0, 0, 0);
            }
        }
        MMK_STAMP(4);
        // ---- epilogue (lanes without an output element store to a sink)
        if constexpr (C8) {
            float v8[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[0][0][r]), __float_as_uint(acc[0][1][r]), false, false);
                const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[0][2][r]), __float_as_uint(acc[0][3][r]), false, false);
                // s..[0]: channels 0-3 of n-tiles (0,1) / (2,3) in lanes 0-31; s..[1]: channels 4-7
                const auto lo = __builtin_amdgcn_permlane32_swap(s01[0], s23[0], false, false);
                const auto hi = __builtin_amdgcn_permlane32_swap(s01[1], s23[1], false, false);
                v8[r] = __uint_as_float(lo[0]);
                v8[4 + r] = __uint_as_float(hi[0]);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) v8[r] = fmaxf(__builtin_fmaf(v8[r], dk, bs8[r]), relu_lo);
            if (dp.thr != 0u) {
                const unsigned e4 = (unsigned)pix0 * 8u + __umul24((unsigned)lpix8, 8u);
                bool kp[4];
                dropout_keep4(a.seed, e4, dp, kp);
#pragma unroll
                for (int r = 0; r < 4; ++r) v8[r] = kp[r] ? v8[r] : 0.f;
                dropout_keep4(a.seed, e4 + 4u, dp, kp);
#pragma unroll
                for (int r = 0; r < 4; ++r) v8[4 + r] = kp[r] ? v8[4 + r] : 0.f;
            }
            if constexpr (EPI) {
                float sv[8], av[8];
                unpack8(e8_src, sv);
                unpack8(e8_acc, av);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float masked = (sv[r] > 0.f) ? v8[r] * c8_scale : 0.f;
                    v8[r] = c8_has_src ? masked : v8[r];
                    v8[r] += av[r];                          // zeros unless accumulating
                }
            }
            const bool ok8 = (ty0 + lrow8) < a.H && (tx0 + lcol8) < a.W;
            u32x4 *dst8 = ok8 ? reinterpret_cast<u32x4 *>(a.o1.y + (pix0 + lpix8) * 8) : reinterpret_cast<u32x4 *>(g_sink16);
            if (MMK_RING_DIAG != 1 || a.seed == 0x7fffffffu) *dst8 = pack8(v8);
        } else {
        float pv[POOL == 1 ? MT : 1][2][4]; // POOL 1: maximum over the wave's two tile rows, per 16-pixel half
        unsigned pr[POOL == 2 ? MT : 1][NT][2]; // POOL 2: the lane's outputs as the full-resolution tensor would store them: bf16 pairs
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const bool okp = (ty0 + 2 * wv + (n >> 1)) < a.H && (tx0 + (n & 1) * 16 + (lane & 15)) < a.W;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if constexpr (!EPI && POOL != 1) {
                    // Forward roles (round 5): the lane's four values as two packed bf16 pairs -- fma (dropout's keep factor
                    // folded into the bias), v_cvt_pk_bf16_f32, ReLU as v_pk_max_i16 on the bit patterns (relu_pk = 0, or
                    // -32768 = identity), the dropout mask as saturating packed subtract + arithmetic shift of the two hash
                    // words: 12 + 14 instead of 12 + 26 vector instructions per four values beside the hash.
                    unsigned pq[2];
#pragma unroll
                    for (int hlf = 0; hlf < 2; ++hlf)
                        pq[hlf] = pk_max_i16(cvt_pk_bf16(__builtin_fmaf(acc[m][n][2 * hlf], dk, bs[m][2 * hlf]),
                                                         __builtin_fmaf(acc[m][n][2 * hlf + 1], dk, bs[m][2 * hlf + 1])), relu_pk);
                    if (dp.thr != 0u) {
                        unsigned hw0, hw1;
                        dropout_words(a.seed, (unsigned)pix0 * (unsigned)a.COUT + __umul24((unsigned)lane_pix[n], (unsigned)a.COUT) +
                                                  (unsigned)o_e0[m], hw0, hw1);
                        pq[0] &= pk_keep_mask(hw0, thr1pk);
                        pq[1] &= pk_keep_mask(hw1, thr1pk);
                    }
                    if constexpr (POOL == 2) {
                        pr[m][n][0] = pq[0];
                        pr[m][n][1] = pq[1];
                    } else {
                        unsigned long long *dst = (okp && o_cv[m]) ? reinterpret_cast<unsigned long long *>(o_yb[m] + (pix0 * o_C[m] + o_loff[m][n]))
                                                                   : reinterpret_cast<unsigned long long *>(g_sink16);
                        if (MMK_RING_DIAG != 1 || a.seed == 0x7fffffffu) *dst = (unsigned long long)pq[0] | ((unsigned long long)pq[1] << 32);
                    }
                    continue;
                }
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(__builtin_fmaf(acc[m][n][r], dk, bs[m][r]), relu_lo);
                if (dp.thr != 0u) {
                    bool kp[4];
                    // element index (pixel * COUT + channel) mod 2^32: the tile origin's product is scalar, the
                    // in-tile pixel offset fits 24 bits
                    dropout_keep4(a.seed, (unsigned)pix0 * (unsigned)a.COUT + __umul24((unsigned)lane_pix[n], (unsigned)a.COUT) +
                                              (unsigned)o_e0[m], dp, kp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = kp[r] ? v[r] : 0.f;
                }
                if constexpr (EPI) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float masked = ((float)e_src[m][n][r] > 0.f) ? v[r] * o_scale[m] : 0.f;
                        v[r] = o_has_src[m] ? masked : v[r];
                        v[r] += (float)e_acc[m][n][r];       // zeros unless accumulating
                    }
                }
                if constexpr (POOL == 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pv[m][n & 1][r] = (n < 2) ? v[r] : fmaxf(pv[m][n & 1][r], v[r]);
                }
                bf16x4 outv;
#pragma unroll
                for (int r = 0; r < 4; ++r) outv[r] = (bf16)v[r];
                if constexpr (POOL == 2) {
                    // (pixels outside the image take no part in a stored window: floor pooling)
                    const unsigned long long pk = __builtin_bit_cast(unsigned long long, outv);
                    pr[m][n][0] = (unsigned)pk;
                    pr[m][n][1] = (unsigned)(pk >> 32);
                } else {
                    bf16x4 *dst = (okp && o_cv[m]) ? reinterpret_cast<bf16x4 *>(o_yb[m] + (pix0 * o_C[m] + o_loff[m][n]))
                                                   : reinterpret_cast<bf16x4 *>(g_sink16);
                    *dst = outv;
                }
            }
        }
        if constexpr (POOL == 2) {
            // The window of pooled pixel (wv, 8 hsel + l%16 / 2): rows = the wave's two tile rows (n-tiles h and 2 + h of half h),
            // columns = this lane and its neighbour l ^ 1 (even lane = left).  The even lane of a pair stores the first
            // 16-pixel half's window, the odd lane the second half's (all 64 lanes store, to distinct addresses).  The
            // arg-max is taken on the values as the full-resolution tensor would have stored them (rounded to bf16), first
            // maximum in scan order -- what maxpool2_bwd_kernel finds in the stored tensor.  The outputs are >= +0 (ReLU,
            // dropout), so their bf16 patterns order like 15-bit integers: the tournament (left vs right per row, then row 0 vs
            // row 1, strict comparisons = first maximum) runs on packed pairs with 16-bit integer instructions.
            typedef short s16x2 __attribute__((ext_vector_type(2)));
            typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
            const int hsel = lane & 1;
            const bool okq = ((ty0 >> 1) + wv) < Hp && ((tx0 >> 1) + hsel * 8 + ((lane & 15) >> 1)) < Wp;
            auto gt_mask = [](unsigned a, unsigned b) {        // per 16-bit half: 0xFFFF where b > a
                const s16x2 d = __builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b);
                return __builtin_bit_cast(unsigned, (s16x2)(d >> 15));
            };
            auto max2 = [](unsigned a, unsigned b) {
                return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
            };
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                unsigned outp[2], code = 0;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const unsigned x0 = hsel ? pr[m][1][q] : pr[m][0][q], x1 = hsel ? pr[m][3][q] : pr[m][2][q];   // mine, my half
                    const unsigned y0 = hsel ? pr[m][0][q] : pr[m][1][q], y1 = hsel ? pr[m][2][q] : pr[m][3][q];   // mine, the neighbour's half
                    const unsigned n0 = (unsigned)__builtin_amdgcn_mov_dpp((int)y0, 0xB1, 0xF, 0xF, true);
                    const unsigned n1 = (unsigned)__builtin_amdgcn_mov_dpp((int)y1, 0xB1, 0xF, 0xF, true);
                    const unsigned l0 = hsel ? n0 : x0, r0 = hsel ? x0 : n0, l1 = hsel ? n1 : x1, r1 = hsel ? x1 : n1;
                    const unsigned g0 = gt_mask(l0, r0), g1 = gt_mask(l1, r1);
                    const unsigned m0 = max2(l0, r0), m1 = max2(l1, r1);
                    const unsigned g2 = gt_mask(m0, m1);
                    const unsigned mx = max2(m0, m1);
                    const unsigned a0 = g0 & 0x00010001u, a1 = (g1 & 0x00010001u) | 0x00020002u;
                    const unsigned arg = (a0 & ~g2) | (a1 & g2);
                    const unsigned one = 0x00010001u;
                    const unsigned pos = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, mx), __builtin_bit_cast(u16x2, one)));
                    const unsigned c = arg | (pos << 2);                   // a 4-bit code in each 16-bit half
                    outp[q] = mx;
                    code |= ((c & 0xFu) | ((c >> 12) & 0xF0u)) << (8 * q);
                }
                const bool okm = okq && o_cv[m];
                unsigned long long *dstp = okm ? reinterpret_cast<unsigned long long *>(a.pool_y + (pp0 * a.COUT + p_loff[m]))
                                               : reinterpret_cast<unsigned long long *>(g_sink16);
                *dstp = (unsigned long long)outp[0] | ((unsigned long long)outp[1] << 32);
                unsigned short *dsta = okm ? reinterpret_cast<unsigned short *>(a.pool_arg + ((pp0 * a.COUT + p_loff[m]) >> 1))
                                           : reinterpret_cast<unsigned short *>(g_sink16);
                *dsta = (unsigned short)code;
            }
        }
        if constexpr (POOL == 1) {
            // rounding to bf16 is monotonic: the maximum of the fp32 values rounds to the maximum of the
            // stored ones.  After the horizontal maximum both lanes of a pixel pair hold the pooled value of
            // either 16-pixel half: the even lane stores the first half's, the odd lane the second half's —
            // all 64 lanes store, to distinct addresses (parking the odd lanes on the sink made 32 lanes hit
            // one address per store: +75 % on the 640x640 level).
            const int hsel = lane & 1;
            const bool okq = ((ty0 >> 1) + wv) < Hp && ((tx0 >> 1) + hsel * 8 + ((lane & 15) >> 1)) < Wp;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                bf16x4 outp;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p0 = pv[m][0][r], p1 = pv[m][1][r];
                    const float n0 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(p0), 0xB1, 0xF, 0xF, true));
                    const float n1 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(p1), 0xB1, 0xF, 0xF, true));
                    outp[r] = (bf16)(hsel ? fmaxf(p1, n1) : fmaxf(p0, n0));
                }
                bf16x4 *dstp = (okq && o_cv[m]) ? reinterpret_cast<bf16x4 *>(a.pool_y + (pp0 * a.COUT + p_loff[m]))
                                                : reinterpret_cast<bf16x4 *>(g_sink16);
                *dstp = outp;
            }
        }
        }   // !C8
        MMK_STAMP(5);
#ifdef MMK_DEEP_STAMPS
        ++stamp_stage;
#endif
    }
}
