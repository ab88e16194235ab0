// bwd_split_body.inc -- the body of interact_bwd_split_kernel and interact_bwd_split_lo_kernel (interact.hip,
// where the load plan is described), included inside each kernel's braces.  In scope: T, NB, DC, SPB, WPS,
// MAPPED, CPL, YS, the kernel's arguments, and SU = the type of `su` (StepUpdate: Descent's once-hit write;
// SplitStepUpdate: the split rule's, whose branches are `if constexpr (SU::kSplit)`; AdagradStepUpdate: the
// Adagrad rules', whose branches are `if constexpr (AG == 1)`, the element-wise rule, and `(AG == 2)`, the
// row-wise one).
    static_assert(CPL == 4 || (CPL == 8 && sizeof(T) == 2), "8 columns per lane: bf16 rows");
    static_assert(!SU::kSplit || (sizeof(T) == 2 && !YS && !MAPPED), "split rows live in bf16 tables");
    constexpr int AG = step_adagrad_kind((const SU*)nullptr);
    static_assert(AG == 0 || (!YS && !MAPPED), "the Adagrad rules step the training step's tables");
    // the row-wise sum of squares crosses the sample's two waves once: one super-block per wave, so the block
    // barrier of that exchange sits in uniform control flow
    static_assert(AG != 2 || WPS == 1 || DC == 128, "row-wise over two waves: d = 128");
    constexpr int NS = 16 * NB;
    constexpr int KS = 4 * NB;
    constexpr int PMAX = NS * (NS - 1) / 2;
    constexpr int SBC = 16 * CPL;  // columns per super-block
    // the wave's tile of T: fp32 (CPL = 4) or the rows' own bf16 (CPL = 8)
    typedef typename std::conditional<CPL == 8, uint16_t, float>::type TileT;
    const int d = DC > 0 ? DC : d_;
    __shared__ float pk_all[SPB][PMAX];  // each sample's packed gradient row
    // each wave's tile of T (the once-hit update reads it; YS has none)
    __shared__ __attribute__((aligned(16))) TileT tt_all[YS ? 1 : WPS * SPB][YS ? 4 : NS * SBC];
    __shared__ TableDesc tds[YS ? 1 : NS];
    __shared__ int64_t dmap[MAPPED ? 2 * NS : 1];  // table t's dt rows at dt + dmap[t] + b * dmap[F - 1 + t]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = w / WPS, h = w % WPS;
    constexpr bool mapped = MAPPED;
    const int c = lane & 15, q = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * SPB + pair;
    const bool live = b < B;
    const int64_t bb = live ? b : 0;  // a padding sample reads sample 0 (and stores nothing)
    const int ksteps = (F + 3) / 4;
    const int P = F * (F - 1) / 2;
    const T* ob = dout + bb * dout_ld;
    float* pk = pk_all[pair];
    TileT* Tt = tt_all[YS ? 0 : w];
    if (h == 0) WT(1, 0, b);
    // the table descriptors (F - 1 <= NS <= 32 < blockDim: one per thread), held in registers and
    // written to LDS after the other independent loads are issued, so no wave waits for them alone
    const bool tdl_ok = !YS && (int)threadIdx.x < F - 1;
    const TableDesc tdl = YS ? TableDesc{nullptr, 0} : load_table(ga.tabs, tdl_ok ? (int)threadIdx.x : 0);
    int64_t dm0 = 0, dm1 = 0;
    if constexpr (MAPPED) {
        dm0 = ldg<int64_t>(ga.dtb + (tdl_ok ? threadIdx.x : 0));
        dm1 = ldg<int64_t>(ga.dtl + (tdl_ok ? threadIdx.x : 0));
    }
    // ---- every independent load first: table `lane`'s index and flag, the packed gradients, x part
    const bool tl = !YS && lane < F - 1;
    const int64_t myidx = YS ? 0 : load_index_if(tl, ga.idx, ga.itype, (int64_t)(tl ? lane : 0) * ga.tstride + bb);
    // su.single NULL (dlrm_interact_bwd_blocked, YS): no once-hit update, every table row goes to dt
    const uint8_t myfl = su.single ? ldg<uint8_t>(su.single + (tl ? (int64_t)lane * su.cap + bb : 0)) : (uint8_t)0;
    // split: the tables' low-half pointers reach the writing lanes through LDS, beside tds (d = 128: the
    // forms with 256 B of LDS to spare at their occupancy), else as the rows do, by shuffle from lane t
    constexpr bool LO_LDS = DC == 128;
    long long mylo = 0;
    uint16_t** lop = nullptr;
    if constexpr (SU::kSplit) {
        if constexpr (LO_LDS) {
            lop = lo_tab<NS>();
            mylo = (long long)ldg<uint16_t*>(step_lo(su) + (tdl_ok ? threadIdx.x : 0));
        } else {
            mylo = (long long)ldg<uint16_t*>(step_lo(su) + (tl ? lane : 0));
        }
    }
    // Adagrad: the tables' state pointers travel the same two ways
    long long myst = 0;
    float** sop = nullptr;
    if constexpr (AG != 0) {
        if constexpr (LO_LDS) {
            sop = state_tab<NS>();
            myst = (long long)ldg<float*>(step_state(su) + (tdl_ok ? threadIdx.x : 0));
        } else {
            myst = (long long)ldg<float*>(step_state(su) + (tl ? lane : 0));
        }
    }
    constexpr int PPW = (PMAX + 64 * WPS - 1) / (64 * WPS);  // packed values staged per lane
    float pv[PPW];
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 64 * WPS * k;
        const float v = to_f32(ldg<T>(ob + d + (p < P ? p : 0)));
        pv[k] = p < P ? v : 0.0f;
    }
    // super-blocks per wave (CPL = 4, WPS = 2: d <= 512 when not fixed; WPS = 1: d <= 64;
    // CPL = 8: d <= 128, one wave)
    // (DC = 0: WPS = 1 / 2 cover d <= 64 / 512; YS: d = 64 * WPS, one super-block per wave)
    constexpr int SBW = YS ? 1
                           : DC > 0 ? ((DC / SBC + WPS - 1) / WPS > 0 ? (DC / SBC + WPS - 1) / WPS : 1)
                                    : (WPS == 2 ? 4 : 1);
    constexpr int XV = SBC / 64;  // dout x-part values per lane and super-block
    float xv[SBW][XV];
#pragma unroll
    for (int sbi = 0; sbi < SBW; ++sbi)
#pragma unroll
        for (int k = 0; k < XV; ++k) {
            const int n = SBC * h + SBC * WPS * sbi + 64 * k + lane;
            xv[sbi][k] = to_f32(ldg<T>(ob + (n < d ? n : 0)));
        }
    const bool frozen = su.single ? *su.err != 0 : true;  // a bounds error this step: no table row is written
    if (su.single && blockIdx.x == 0 && threadIdx.x == 0) snapshot_error(su.err, frozen ? 1u : 0u);
    if (tdl_ok) {
        tds[threadIdx.x] = tdl;
        if constexpr (SU::kSplit && LO_LDS) lop[threadIdx.x] = (uint16_t*)mylo;
        if constexpr (AG != 0 && LO_LDS) sop[threadIdx.x] = (float*)myst;
        if constexpr (MAPPED) {
            dmap[threadIdx.x] = dm0;
            dmap[F - 1 + threadIdx.x] = dm1;
        }
    }
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 64 * WPS * k;
        if (p < PMAX) pk[p] = pv[k];
    }
    __syncthreads();  // tds, pk
    // validate this lane's table index; rows travel as 32-bit (~0u = invalid / no table)
    uint32_t myrow = ~0u;
    if (tl) {
        const int64_t r = myidx - ga.base;
        if (r >= 0 && r < tds[lane].nrows) myrow = (uint32_t)r;
        else if (h == 0 && live) raise_index_error(ga.err);
    }
    const T* rowp[KS];
    unsigned livek = 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = 4 * s + q;
        const uint32_t r = (uint32_t)__shfl((int)myrow, kk >= 1 ? kk - 1 : 0, 64);
        const bool tab = s < ksteps && kk >= 1 && kk < F && r != ~0u;
        const T* src = YS ? ((s < ksteps && kk < F) ? x + bb * x_ld + (int64_t)kk * d : nullptr)
                   : (s < ksteps && kk == 0) ? x + bb * x_ld
                                             : (tab ? (const T*)tds[kk - 1].data + (int64_t)r * d : nullptr);
        livek |= src ? (1u << s) : 0u;
        // (CPL = 8: a masked row reads the zero row -- a 16-B aligned source whatever dout's layout)
        rowp[s] = src ? src : (CPL == 8 ? (const T*)g_zero_row : ob);
    }
    uint32_t urow[NB][4];
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = I * 16 + 4 * q + r;
            const int src = (f >= 1 && f < F) ? f - 1 : 0;
            const uint32_t row = (uint32_t)__shfl((int)myrow, src, 64);
            const int fl = __shfl((int)myfl, src, 64);
            urow[I][r] = (f >= 1 && f < F && !frozen && fl != 0) ? row : ~0u;
        }
    if (h == 0) WT(1, 1, b);
#pragma unroll
    for (int sbi = 0; sbi < SBW; ++sbi) {
        const int sb = SBC * h + SBC * WPS * sbi;
        if (sb >= d) break;
        const int n0 = sb + CPL * c;  // this lane's CPL output columns
        const bool colok = n0 < d;
        const int nc = colok ? n0 : 0;
        f32x4_t acc[NB][CPL];
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int e = 0; e < CPL; ++e) acc[I][e] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if constexpr (CPL == 4) {
            f32x4_t bv[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const f32x4_t v = load4_f32(rowp[s] + nc);
                bv[s] = ((livek >> s) & 1u) && colok ? v : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            if (sbi > 0) wave_lds_sync();  // the previous super-block's tile reads are done
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (s < ksteps) *(f32x4_t*)(Tt + (4 * s + q) * SBC + 4 * c) = bv[s];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < ksteps) {
                    const int kk = 4 * s + q;
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        // S[16I+c][kk]: the symmetric zero-diagonal unpack of the pair row
                        const int i = I * 16 + c;
                        const int hi = i > kk ? i : kk, lo = i > kk ? kk : i;
                        const float av = (i != kk && hi < F) ? pk[hi * (hi - 1) / 2 + lo] : 0.0f;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[s][e], acc[I][e], 0, 0, 0);
                    }
                }
            }
        } else {
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            u32x4_t bv[KS];  // 8 bf16 columns of row 4s+q, packed
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4_t v = ldg<u32x4_t>(rowp[s] + nc);
                bv[s] = ((livek >> s) & 1u) && colok ? v : u32x4_t{0u, 0u, 0u, 0u};
            }
            if (sbi > 0) wave_lds_sync();  // the previous super-block's tile reads are done
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (s < ksteps) *(u32x4_t*)(Tt + (4 * s + q) * SBC + 8 * c) = bv[s];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < ksteps) {
                    const int kk = 4 * s + q;
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        const int i = I * 16 + c;
                        const int hi = i > kk ? i : kk, lo = i > kk ? kk : i;
                        const float av = (i != kk && hi < F) ? pk[hi * (hi - 1) / 2 + lo] : 0.0f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const uint32_t wd = bv[s][e >> 1];
                            const float bvf = __uint_as_float((e & 1) ? (wd & 0xffff0000u) : (wd << 16));
                            acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bvf, acc[I][e], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (h == 0 && sbi == 0) WT(1, 2, b);
        // dout's x part for this lane's columns (lanes 0..15 hold output row 0)
        float xo[CPL];
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            const int n = CPL * c + e;  // column within the super-block: lane n & 63 of xv[sbi][n >> 6]
            float xs = __shfl(xv[sbi][0], n & 63, 64);
#pragma unroll
            for (int k = 1; k < XV; ++k) {
                const float t = __shfl(xv[sbi][k], n & 63, 64);
                xs = (n >> 6) == k ? t : xs;
            }
            xo[e] = xs;
        }
        wave_lds_sync();  // the tile of T (written before the MFMAs)
        // split, pointers by shuffle: here, in uniform control flow and after the MFMAs (held through them, with
        // the gathered rows in flight, they cost the one-wave form registers it does not have at 32 features)
        uint16_t* ulo[NB][4];
        if constexpr (SU::kSplit && !LO_LDS) {
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = I * 16 + 4 * q + r;
                    ulo[I][r] = (uint16_t*)__shfl(mylo, (f >= 1 && f < F) ? f - 1 : 0, 64);
                }
        }
        float* ust[NB][4];
        if constexpr (AG == 1 && !LO_LDS) {
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = I * 16 + 4 * q + r;
                    ust[I][r] = (float*)__shfl(myst, (f >= 1 && f < F) ? f - 1 : 0, 64);
                }
        }
        // (row-wise: its shuffles and its block barrier need uniform control flow, so padding samples and lanes
        // past the row come along into the loop and leave it per tile row, after the row sums)
        if constexpr (AG != 2) {
            if (!live || !colok) continue;
        }
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            // split: the low halves of this lane's once-hit rows among the four of tile row I (its CPL columns),
            // loaded together before the first of them is written (8 columns per lane: each at its write --
            // four 16-B vectors would take that form from 6 to 4 waves per SIMD at 16 features).  Issued
            // behind the gathered rows they would travel beside the gather, but waiting as bits through the
            // MFMAs they took the two-wave form from 8 to 6 waves per SIMD at 16 features and spilt at 32.
            auto lo_row = [&](int r) {
                const int f = I * 16 + 4 * q + r;
                uint16_t* base;
                if constexpr (LO_LDS) base = lop[f - 1];
                else base = ulo[I][r];
                return base + (int64_t)urow[I][r] * d + n0;
            };
            typename Halves<CPL>::type lov[4];
            if constexpr (SU::kSplit && CPL == 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u) lov[r] = load_halves<CPL>(lo_row(r));
            }
            // Adagrad: the state of this lane's once-hit rows, loaded here as the low halves are (after the
            // MFMAs, the four of a tile row together) -- the element-wise rule's fp32 state row at the lane's
            // columns (8 columns per lane: each at its write), the row-wise rule's word
            // (with up to 16 features the state is loaded at each row's write instead: four in flight took the
            // NB = 1 forms below Descent's 8 waves per SIMD)
            constexpr bool ST4 = NB > 1 && CPL == 4;
            float* usr[4];  // the four tables' state pointers (by shuffle)
            if constexpr (AG == 1 && !LO_LDS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) usr[r] = ust[I][r];
            }
            // row-wise: the four tile rows' sums of squares of G = 0 + g, in the order of the apply's once-hit item
            // (apply.hpp run_singles, fp32 gradient rows: apply lane v holds columns 4v..4v+3) -- a lane's fma
            // chain from 0 over four columns in column order, then the xor butterfly over the row's lanes from
            // distance 1 up.  Lane c holds apply lane 16h + c's columns (8 columns per lane: lanes 2c and 2c + 1,
            // so its two chains' sum is level 1 and the butterfly over c levels 2..16); a lane past the row
            // (!colok: its accumulators are 0) adds +0, which keeps the bits of a sum >= 0.  d = 128 over two
            // waves: each wave's 64 columns over c, then the last level, one commutative add of the two waves'
            // totals, through LDS (a slot per tile row I: one barrier each, nothing is overwritten).
            // The state word m of a row is one address for both waves, and wave 0 stores m' there: so only wave 0
            // ever loads it (its c == 0 lanes, before the barrier) and hands it to both waves through the same LDS
            // exchange.  Wave 1 never reads a word that wave 0 writes.
            float rs[4];
            float mx[4];  // two waves: the rows' state words, out of LDS
            if constexpr (AG == 2) {
                float m0w[4];
                if constexpr (WPS == 2) {
                    if (h == 0 && c == 0 && live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int f = I * 16 + 4 * q + r;
                            if (f < F && urow[I][r] != ~0u) m0w[r] = ldg<float>(sop[f - 1] + urow[I][r]);
                        }
                    }
                }
                if constexpr (!LO_LDS) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = I * 16 + 4 * q + r;
                        usr[r] = (float*)__shfl(myst, (f >= 1 && f < F) ? f - 1 : 0, 64);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float g[CPL];
#pragma unroll
                    for (int e = 0; e < CPL; ++e) g[e] = 0.0f + acc[I][e][r];
                    float ss = sum_squares<4>(g, 0.0f);
                    if constexpr (CPL == 8) ss += sum_squares<4>(g + 4, 0.0f);
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);
                    rs[r] = ss;
                }
                if constexpr (WPS == 2) {
                    float* sx = row_ss_tab<SPB * 3 * NS>();  // [SPB][wave 0's sums, wave 1's sums, m][NS]
                    if (c == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) sx[(pair * 3 + h) * NS + I * 16 + 4 * q + r] = rs[r];
                        if (h == 0 && live) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int f = I * 16 + 4 * q + r;
                                if (f < F && urow[I][r] != ~0u) sx[(pair * 3 + 2) * NS + f] = m0w[r];
                            }
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        rs[r] += sx[(pair * 3 + (h ^ 1)) * NS + I * 16 + 4 * q + r];
                        mx[r] = sx[(pair * 3 + 2) * NS + I * 16 + 4 * q + r];
                    }
                }
                if (!live || !colok) continue;
            }
            auto st_base = [&](int r) {
                const int f = I * 16 + 4 * q + r;
                float* base;
                if constexpr (LO_LDS) base = sop[f - 1];
                else base = usr[r];
                return base;
            };
            f32x4_t sv[AG == 1 && ST4 ? 4 : 1];
            float mv[AG == 2 && ST4 && WPS == 1 ? 4 : 1];
            if constexpr (AG == 1 && ST4) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u)
                        sv[r] = ldg<f32x4_t>(st_base(r) + (int64_t)urow[I][r] * d + n0);
            }
            if constexpr (AG == 2 && ST4 && WPS == 1) {  // (one wave holds the row: its own loads, then its store)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u) mv[r] = ldg<float>(st_base(r) + urow[I][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = I * 16 + 4 * q + r;
                if (f < F) {
                    float v[CPL];
#pragma unroll
                    for (int e = 0; e < CPL; ++e) v[e] = acc[I][e][r];
                    if (urow[I][r] != ~0u) {
                        float wv[CPL];
                        float tw[CPL];  // the row as gathered
                        if constexpr (CPL == 4) {
                            const f32x4_t t4 = *(const f32x4_t*)(Tt + f * SBC + 4 * c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) tw[e] = t4[e];
                        } else {
                            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
                            const u32x4_t t8 = *(const u32x4_t*)(Tt + f * SBC + 8 * c);
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                tw[e] = __uint_as_float((e & 1) ? (t8[e >> 1] & 0xffff0000u) : (t8[e >> 1] << 16));
                        }
                        if constexpr (SU::kSplit) {
                            // (either tile layout gives the element's bf16 bits << 16 exactly)
                            const int64_t ro = (int64_t)urow[I][r] * d + n0;
                            uint32_t hb[CPL];
#pragma unroll
                            for (int e = 0; e < CPL; ++e) hb[e] = __float_as_uint(tw[e]);
                            if constexpr (CPL == 8) lov[r] = load_halves<CPL>(lo_row(r));
                            split_once_hit<CPL>(su.lr, v, hb, lov[r], (uint16_t*)tds[f - 1].data + ro, lo_row(r));
                        } else if constexpr (AG == 1) {
                            // A += G^2, w -= lr G / (sqrt(A) + eps) with G = 0 + g: apply.hpp's adagrad_step
                            float* srow = st_base(r) + (int64_t)urow[I][r] * d + n0;
                            float gg[CPL], av[CPL];
#pragma unroll
                            for (int e = 0; e < CPL; e += 4) {
                                f32x4_t a4;
                                if constexpr (ST4) a4 = sv[r];
                                else a4 = ldg<f32x4_t>(srow + e);
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    av[e + k] = a4[k];
                                    gg[e + k] = 0.0f + v[e + k];
                                }
                            }
                            adagrad_step<CPL>(su.lr, step_eps(su), gg, av, tw);
#pragma unroll
                            for (int e = 0; e < CPL; e += 4)
                                stg_nt<f32x4_t>(srow + e, f32x4_t{av[e], av[e + 1], av[e + 2], av[e + 3]});
                            store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, tw);
                        } else if constexpr (AG == 2) {
                            // m += ss / D, w -= (lr / (sqrt(m) + eps)) G: apply.hpp's helpers, one lane stores m
                            float m0;
                            if constexpr (WPS == 2) m0 = mx[r];
                            else if constexpr (ST4) m0 = mv[r];
                            else m0 = ldg<float>(st_base(r) + urow[I][r]);
                            const float m = rowwise_m(m0, rs[r], d);
                            const float sc = rowwise_scale(su.lr, step_eps(su), m);
#pragma unroll
                            for (int e = 0; e < CPL; ++e) wv[e] = __builtin_fmaf(-sc, 0.0f + v[e], tw[e]);
                            store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, wv);
                            if (c == 0 && h == 0) stg<float>(st_base(r) + urow[I][r], m);
                        } else {
#pragma unroll
                        for (int e = 0; e < CPL; ++e) wv[e] = __builtin_fmaf(-su.lr, 0.0f + v[e], tw[e]);
                        store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, wv);
                        }
                    } else if (!mapped && (f > 0 || !su.single)) {
                        // (the training step (su.single set) leaves dt's x row alone: dx carries it)
                        // (CPL = 8: a lane's two 16-B pieces are 32 B apart, so each store instruction
                        // covers half of every line: plain stores let L2 merge the halves, where
                        // non-temporal ones left as partial-line writes, 95 -> 117 MB per launch)
#pragma unroll
                        for (int e = 0; e < CPL; e += 4) {
                            const f32x4_t pv4 = f32x4_t{v[e], v[e + 1], v[e + 2], v[e + 3]};
                            if constexpr (CPL == 8) stg<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0 + e, pv4);
                            else stg_nt<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0 + e, pv4);
                        }
                    } else if (f > 0) {
#pragma unroll
                        for (int e = 0; e < CPL; e += 4)
                            stg_nt<f32x4_t>(dt + dmap[f - 1] + b * dmap[F - 2 + f] + n0 + e,
                                            f32x4_t{v[e], v[e + 1], v[e + 2], v[e + 3]});
                    }
                    if (f == 0)
#pragma unroll
                        for (int e = 0; e < CPL; e += 4)
                            stg<f32x4_t>(dx + b * dx_ld + n0 + e, f32x4_t{xo[e] + v[e], xo[e + 1] + v[e + 1],
                                                                         xo[e + 2] + v[e + 2], xo[e + 3] + v[e + 3]});
                }
            }
        }
        if (h == 0 && sbi == 0) {
            WT(1, 3, b);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            WT(1, 4, b);
        }
    }
