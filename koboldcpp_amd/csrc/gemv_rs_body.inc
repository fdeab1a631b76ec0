// gemv_rs_body.inc -- the body of gemv_rs.hip k_gemv_rs, included by that kernel and by k_gemv_qkv_dual (a grid
// holding two launches' workgroups).  In scope: the DecArgs `a` (the kernel's own parameter: a copy or a reference
// would move it to scratch memory), the template names of k_gemv_rs, `lds` (dynamic LDS), KB_BID / KB_NBLK (this
// workgroup's index and the workgroup count of its launch), EX (MODE 2, R = 2 with DecArgs.bias / rope_neox honoured).
    using T = RS<TYPE>;
    constexpr int RR = MODE == 1 ? 2 * R : R;
    static_assert(MODE != 3 || (NWV == 8 && PRO == 2 && !ROUTE), "MODE 3: 8 waves, quantize prologue");
#ifdef KCPP_STAMPS
    __shared__ unsigned long long *st_s;
    if (threadIdx.x == 0) {
        unsigned long long *b = g_rs_stamps;   // every 8th workgroup records (one counter: ~88 adds per us)
        st_s = (b && (KB_BID & 7) == 0) ? b + 16ull * (atomicAdd(&g_rs_slot, 1u) & 131071u) : nullptr;
        if (st_s) {
            st_s[5] = ((unsigned long long)KB_NBLK << 32) | (unsigned)KB_BID;
            st_s[6] = (unsigned long long)a.K | ((unsigned long long)MODE << 24) | ((unsigned long long)PRO << 28);
            st_s[7] = (unsigned long long)(a.N[0] + (a.nseg > 1 ? a.N[1] : 0) + (a.nseg > 2 ? a.N[2] : 0));
        }
    }
    __syncthreads();
    unsigned long long *st_ = st_s;
    RS_STAMP(0);
#endif
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = (int)a.K, nsb = K / 256, RB = nsb * T::BYTES;
    const int npieces = nsb * T::PIECES_PER_SB;
    const int N0 = (int)a.N[0], N1 = a.nseg > 1 ? (int)a.N[1] : 0, N2 = a.nseg > 2 ? (int)a.N[2] : 0;
    const int ngroups = (N0 + N1 + N2) / R;
    constexpr int WPG = MODE == 3 ? NWV / 2 : NWV;     // waves per group set (MODE 3: per expert half)
    const int hx = MODE == 3 ? __builtin_amdgcn_readfirstlane(wave / WPG) : 0;   // MODE 3: which slot this wave serves
    const int nw = KB_NBLK * WPG;
    const int wid = KB_BID * WPG + (MODE == 3 ? wave % WPG : wave);
    int64_t eoff = ROUTE ? 0 : dec_expert_offset(a);   // MoE slice
    int64_t eoff1 = ROUTE ? 0 : (a.eid1 ? dec_expert_offset(a, a.eid1) : eoff);   // segment 1's (two slots in one launch)
    const int abytes = K + K / 256 * 4 + K / 16 * 2;
    const int aoff = MODE == 3 && hx ? (abytes + 15) & ~15 : 0;   // this wave's activation image in LDS
    const typename T::Lane lc = T::lane_consts(lane);

    auto group_rows = [&](int g, int &seg, int &row0) {
        const int r = g * R;
        seg = r < N0 ? 0 : (r < N0 + N1 ? 1 : 2);
        row0 = seg == 0 ? r : (seg == 1 ? r - N0 : r - N0 - N1);
    };
    struct Buf { typename T::W w[NI][RR]; };
    auto issue = [&](int g, Buf &b) {
        int seg, row0;
        group_rows(g, seg, row0);
        int64_t eo = seg == 1 ? eoff1 : eoff;
        if constexpr (MODE == 3) {          // the wave's slot (wave-uniform; a select of the two would go to scratch)
            if (hx) eo = eoff1;
        }
        const uint8_t *W = (seg == 0 ? a.W[0] : (seg == 1 ? a.W[1] : a.W[2])) + eo;
        int rbase = row0, rstride = 1;      // EX: the group's rows (NeoX pairs in the q / k roles, lean::ex_group_rows)
        if constexpr (EX) lean::ex_group_rows(a, seg == 0 ? a.role[0] : (seg == 1 ? a.role[1] : a.role[2]), row0, rbase, rstride);
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int wrow = EX ? rbase + (r % R) * rstride : row0 + (r % R);
            const uint8_t *rp = (MODE == 1 && r >= R ? a.W2 + eo : W) + (int64_t)wrow * RB;
#pragma unroll
            for (int i = 0; i < NI; ++i) T::load(rp, nsb, min(lane + 64 * i, npieces - 1), b.w[i][r]);
        }
    };

    Buf ba, bb;
    const int g0 = min(wid, ngroups - 1);
    if constexpr (PRO != 0) {
        lean::ActPro<PRO, (MC * 4 + NWV - 1) / NWV, 64 * NWV, AUX> pro;
        pro.load(a);
        float4 wpre[ROUTE ? 8 : 1][4];
        const int tid = threadIdx.x;
        if constexpr (ROUTE) {            // router rows first: they do not wait for the norm (k_moe_route's order)
            const bool f16 = a.route_wt == KT_F16;
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = 16 * tid + 4 * u;
                    wpre[e][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (e < a.route_ne && i < K) {
                        if (f16) {
                            const uint2 h = *(const uint2 *)((const uint16_t *)a.route_w + (int64_t)e * K + i);
                            wpre[e][u] = make_float4(h2f(h.x & 0xFFFF), h2f(h.x >> 16), h2f(h.y & 0xFFFF), h2f(h.y >> 16));
                        } else {
                            wpre[e][u] = *(const float4 *)((const float *)a.route_w + (int64_t)e * K + i);
                        }
                    }
                }
        }
        if constexpr (!XL && !ROUTE && MODE != 3) issue(g0, ba);   // XL: a row's pieces and the prologue's registers do not fit together
#ifdef KCPP_STAMPS
        pro.compute(a, lds, st_);
#else
        if constexpr (AUX) pro.compute(a, lds, nullptr, KB_BID == 0 ? auxrn : nullptr, KB_BID == 0 ? auxyn : nullptr);
        else pro.compute(a, lds);
#endif
        if constexpr (MODE == 3) {          // slot 1's h follows slot 0's: its Q8_K image behind the first
            lean::ActPro<PRO, (MC * 4 + NWV - 1) / NWV, 64 * NWV> pro1;
            pro1.load(a, a.K);
            pro1.compute(a, lds + ((abytes + 15) & ~15));
        }
        if constexpr (ROUTE) {
            // logits: thread tid's 16 elements (chunk tid, the prologue's row normalised in pro.v[0]), fma over the
            // 4 float4 in order, wave sums, then ((w0 + w1) + (w2 + w3)) over the first four waves
            __shared__ float r_part[4][8];
            __shared__ int r_id[2];
            __shared__ float r_w[2];
            const bool f16 = a.route_wt == KT_F16;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (16 * tid < K) {
                float xv[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) xv[q] = f16 ? h2f(f2h_rn(pro.v[0][q])) : pro.v[0][q];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e >= a.route_ne) break;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (16 * tid + 4 * u >= K) break;
                        acc[e] = fmaf(xv[4 * u], wpre[e][u].x, acc[e]);
                        acc[e] = fmaf(xv[4 * u + 1], wpre[e][u].y, acc[e]);
                        acc[e] = fmaf(xv[4 * u + 2], wpre[e][u].z, acc[e]);
                        acc[e] = fmaf(xv[4 * u + 3], wpre[e][u].w, acc[e]);
                    }
                }
            }
            if (wave < 4) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e >= a.route_ne) break;
                    const float v = wave_sum(acc[e]);
                    if (lane == 0) r_part[wave][e] = v;
                }
            }
            __syncthreads();
            if (tid == 0) {
                float logit[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    logit[e] = e < a.route_ne ? (r_part[0][e] + r_part[1][e]) + (r_part[2][e] + r_part[3][e]) : 0.0f;
                int id[2];
                float w[2];
                moe_topk8(logit, a.route_ne, 2, id, w);
                r_id[0] = id[0]; r_id[1] = id[1]; r_w[0] = w[0]; r_w[1] = w[1];
                if (KB_BID == 0) {
                    a.route_ids[0] = id[0]; a.route_ids[1] = id[1];
                    a.route_wts[0] = w[0]; a.route_wts[1] = w[1];
                }
            }
            __syncthreads();
            eoff = (int64_t)__builtin_amdgcn_readfirstlane(r_id[0]) * a.ebytes;
            eoff1 = (int64_t)__builtin_amdgcn_readfirstlane(r_id[1]) * a.ebytes;
        }
        if constexpr (XL || ROUTE || MODE == 3) issue(g0, ba);
    } else {
        // the column copy covers K <= 16384 at 256 threads; XL's 512 threads x (4, 3) cover K <= 32768
        lean::ActCopyCol<64 * NWV, XL ? 4 : (16384 / 16 + 64 * NWV - 1) / (64 * NWV), XL ? 3 : (16384 / 256 + 16384 / 32 + 64 * NWV - 1) / (64 * NWV)> cp;
        cp.load(a.act, K, a.act_mtot > 0 ? a.act_mtot : 1, a.act_col);
        issue(g0, ba);
        cp.store(lds, K);
    }
    typename T::Act xr[XL ? 1 : NI];
    if constexpr (!XL) {
#pragma unroll
        for (int i = 0; i < NI; ++i) T::act(lds + aoff, K, min(T::sb_of(lane, i), nsb - 1), lc, xr[i]);
    }
    RS_STAMP(1);
    // MODE 3: waves 4-7 (slot 1's half, the same program as waves 0-3 on the same SIMDs, meeting them in LDS at the
    // end) at static priority 1 -- Mixtral decode 388.4 -> 391.5 tok/s in an alternating A/B, results unchanged
    // (`profiles/r06_gemm_setprio_ab.jsonl`; the dense 8-wave mat-vecs measured slightly slower with it)
    if constexpr (MODE == 3) {
        if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    }

    float slot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) slot[r] = 0.0f;
    // the ggml plugin's fused GLU (AUX instances, MODE 1): gate and up parked beside the product
    constexpr int AUXR = (AUX && MODE == 1) ? R : 1;
    float sgt[AUXR], sup[AUXR];
#pragma unroll
    for (int r = 0; r < AUXR; ++r) { sgt[r] = 0.0f; sup[r] = 0.0f; }
    int slot_g = -1;
    auto compute = [&](int g, const Buf &b, int k) {
        float acc[RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const bool ok = (NI * 64 == npieces) || lane + 64 * i < npieces;
            typename T::Act xl;
            if constexpr (XL) T::act(lds + aoff, K, min(T::sb_of(lane, i), nsb - 1), lc, xl);
#pragma unroll
            for (int r = 0; r < RR; ++r) {
                const float p = T::dot(b.w[i][r], XL ? xl : xr[i], lc);
                acc[r] += ok ? p : 0.0f;
            }
            // XL: keep piece i + 1's LDS activation reads behind piece i's dot (hoisted, all NI of them would be live
            // beside the row's NI in-flight weight pieces and spill)
            if constexpr (XL) asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int r = 0; r < RR; ++r) acc[r] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wave_sum_f(acc[r]))));
        const bool mine = lane == k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v;
            if constexpr (MODE == 1) v = (acc[r] / (1.0f + expf(-acc[r]))) * acc[R + r];
            else v = acc[r];
            slot[r] = mine ? v : slot[r];
            if constexpr (AUX && MODE == 1) {
                sgt[r] = mine ? acc[r] : sgt[r];
                sup[r] = mine ? acc[R + r] : sup[r];
            }
        }
        slot_g = mine ? g : slot_g;
#ifdef KCPP_STAMPS
        if (k == 0) { if (slot[0] == 12345.0f) st_[0] = 0; RS_STAMP(2); }
#endif
    };
    int k = 0;
    if constexpr (PF) {
        for (int g = wid; g < ngroups; g += 2 * nw, k += 2) {
            const int g1 = g + nw, g2 = g + 2 * nw;
            issue(min(g1, ngroups - 1), bb);
            compute(g, ba, k);
            if (g1 >= ngroups) break;
            issue(min(g2, ngroups - 1), ba);
            compute(g1, bb, k + 1);
        }
    } else {
        for (int g = wid; g < ngroups; g += nw, ++k) {
            if (k) issue(g, ba);
            compute(g, ba, k);
        }
    }
    RS_STAMP(3);
    if constexpr (MODE == 3) {
        // the halves meet: lane k of wave w (k-th group of the wave) -> xs[half][w % 4][r][k]; half 0 combines
        __shared__ float xs[2][4][R][64];
#pragma unroll
        for (int r = 0; r < R; ++r) xs[hx][wave % WPG][r][lane] = slot[r];
        __syncthreads();
        if (hx) return;
        const float e0 = a.escale[0], e1 = a.escale[1];
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = __fadd_rn(__fmul_rn(slot[r], e0), __fmul_rn(xs[1][wave][r][lane], e1));
    }
    if (slot_g < 0) return;
    int seg, row0;
    group_rows(slot_g, seg, row0);
    if constexpr (AUX && MODE == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            aux0[row0 + r] = sgt[r];
            aux1[row0 + r] = sgt[r] / (1.0f + expf(-sgt[r]));
            aux2[row0 + r] = sup[r];
        }
    }
    if constexpr (EX) lean::store_group_ex(a, seg, row0, slot);
    else lean::store_group<R, MODE, AUX>(a, seg, row0, slot, aux0, auxh, rp);
#ifdef KCPP_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    RS_STAMP(4);
#endif
