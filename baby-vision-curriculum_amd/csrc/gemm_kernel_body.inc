// Body of gemm_kernel / gemm_det_kernel (gemm.hip), included inside each: one source for the two kernels, each with its own kernel
// argument `g` (a helper function taking the group would copy it to scratch, dynamically indexed).  Expects BM, BN, AT, BT, EARLY_
// and DET in scope.  With BVC_BODY_GATE defined (gemm_gate_kernel) the one epilogue is EPI_RESID_GATE and a `Gate gate` is in scope.
#ifdef BVC_BODY_GATE
#define BVC_IS_RESID(e) ((e) == EPI_RESID_GATE)
#else
#define BVC_IS_RESID(e) ((e) == EPI_RESID)
#endif
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BK = 64;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
    constexpr int DMA_PER_STAGE = BM / 32 + BN / 32;   // LDS-DMA instructions per wave per stage

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    if (BVC_DBG(g, 2) && ((blockIdx.x >> 3) & 1)) __builtin_amdgcn_s_sleep(100);

    // XCD-aware remap (bijective for any grid size): XCD x owns a contiguous run of logical ids
    const int nb = gridDim.x, bid = blockIdx.x;
    const int xq = nb >> 3, xr = nb & 7, xcd = bid & 7;
    int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);

    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxGroup; ++i)
        if (i < g.nprob && lid >= g.tile_start[i]) pi = i;
    const GemmProblem& p = g.prob[pi];
    lid -= g.tile_start[pi];
    // Tile walk inside one problem.  An XCD runs a contiguous run of ids, ~64 of them at a time (32 CUs x 2 workgroups), and
    // whatever those 64 workgroups share must fit its 4 MiB L2:
    //   * K-splits are the SLOWEST index: the workgroups resident together then belong to one split and differ in (m, n), so
    //     they share operand slabs (with the split fastest, 4 of every 4 neighbours shared nothing);
    //   * columns are walked in panels of `panel` tiles, rows fastest-but-one: 64 neighbours form a rows x panel block whose
    //     B panel stays in L2 while the rows stream past it.  Measured before this walk (profiles/r01_d_traffic_b64_dispatches.txt):
    //     encoder fc1 at B=64 fetched 259 MB for 20 MB of operands - its 4.7 MB weight cycled through L2 once per row group.
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int ntiles = tiles_m * tiles_n;
    int split, tm, tn;
    const int G = g.panel[pi];
    if (G > 0) {
        split = lid / ntiles;
        const int t = lid - split * ntiles;
        const int full = (tiles_n / G) * G * tiles_m;          // tiles in the full-width panels
        if (t < full) {
            const int pn = t / (G * tiles_m), w = t - pn * G * tiles_m;
            tm = w / G; tn = pn * G + (w - tm * G);
        } else {
            const int r = tiles_n % G, w = t - full;
            tm = w / r; tn = (tiles_n - r) + (w - tm * r);
        }
    } else {   // legacy walk: split fastest, then along the shorter side of the tile grid
        split = lid % p.split_k;
        const int tl = lid / p.split_k;
        const bool m_fast = tiles_n > tiles_m;
        tm = m_fast ? tl % tiles_m : tl / tiles_n;
        tn = m_fast ? tl / tiles_m : tl % tiles_n;
    }
    const int tile = tm * tiles_n + tn;     // id for the per-tile loss partials (independent of the walk)
    const int m0 = tm * BM, n0 = tn * BN;

    const int nt_all = (p.K + BK - 1) / BK;
    const int per = (nt_all + p.split_k - 1) / p.split_k;
    const int t0 = split * per;
    const int t1 = min(nt_all, t0 + per);
    const int nt = t1 - t0;

    const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.B, p.b_bytes);

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // bias gradient fused into the weight-gradient product: db[m] = sum_k A(m,k) is one more MFMA
    // column against an all-ones operand, computed by the workgroups of the first column tile only
    const bool do_rowsum = AT && p.rowsum != nullptr && n0 == 0 && wn == 0;
    f32x4 accb[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (short)0x3F80;

    // Two K-loop variants, A/B'd in ONE run on one box (profiles/r01_d_kloop_ab.txt; box-to-box variance on the pool is far
    // larger than the effect): the early-refill loop below wins for NN (5-15 %) and TN (~8 %), ties for NT at K <= 768 and wins
    // at long K (enc fc2 22 vs 27 us).  The plain double buffer is kept reachable (stages = 4) for such comparisons.
    constexpr bool EARLY = EARLY_;
    if constexpr (!EARLY) {
        if (nt > 0) {
            stage_tile<BM, AT>(ra, m0, t0 * BK, p.lda, smem, wave, lane);
            stage_tile<BN, BT>(rb, n0, t0 * BK, p.ldb, smem + A_BYTES, wave, lane);
        }
        for (int it = 0; it < nt; ++it) {
            // every wave drains its own DMA, then the barrier publishes the tile and proves the other slot is drained
            wait_vmcnt<0>();
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (it + 1 < nt) {
                char* nxt = smem + ((it + 1) & 1) * STAGE;
                stage_tile<BM, AT>(ra, m0, (t0 + it + 1) * BK, p.lda, nxt, wave, lane);
                stage_tile<BN, BT>(rb, n0, (t0 + it + 1) * BK, p.ldb, nxt + A_BYTES, wave, lane);
            }
            const char* la = smem + (it & 1) * STAGE;
            const char* lb = la + A_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[TM], bfr[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) af[i] = read_frag<BM, AT>(la, wm * WM + 16 * i, ks, lane);
#pragma unroll
                for (int j = 0; j < TN; ++j) bfr[j] = read_frag<BN, BT>(lb, wn * WN + 16 * j, ks, lane);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                if (do_rowsum) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[i], accb[i], 0, 0, 0);
                }
            }
        }
    } else {
        // K loop, "early refill": every wave first pulls ALL its fragments of the current K-step into registers, a barrier
        // proves the slot is drained, the slot is refilled by LDS-DMA at once (K-step t+2) and only then do the MFMAs run -
        // from registers.  Two K-steps of DMA are in flight during the MFMAs with just two 32 KiB slots (the plain double
        // buffer had one, and rocprofv3 showed ~50 % of wave cycles waiting on it), so 2 workgroups still fit per CU.
        if (nt > 0) {
            stage_tile<BM, AT>(ra, m0, t0 * BK, p.lda, smem, wave, lane);
            stage_tile<BN, BT>(rb, n0, t0 * BK, p.ldb, smem + A_BYTES, wave, lane);
            if (nt > 1) {
                stage_tile<BM, AT>(ra, m0, (t0 + 1) * BK, p.lda, smem + STAGE, wave, lane);
                stage_tile<BN, BT>(rb, n0, (t0 + 1) * BK, p.ldb, smem + STAGE + A_BYTES, wave, lane);
                wait_vmcnt<DMA_PER_STAGE>();
            } else {
                wait_vmcnt<0>();
            }
            asm volatile("s_barrier" ::: "memory");
        }
        for (int it = 0; it < nt; ++it) {
            char* slot = smem + (it & 1) * STAGE;
            bf16x8 af[2][TM], bfr[2][TN];
    #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
    #pragma unroll
                for (int i = 0; i < TM; ++i) af[ks][i] = read_frag<BM, AT>(slot, wm * WM + 16 * i, ks, lane);
    #pragma unroll
                for (int j = 0; j < TN; ++j) bfr[ks][j] = read_frag<BN, BT>(slot + A_BYTES, wn * WN + 16 * j, ks, lane);
            }
            auto mfma_half = [&](int ks) {
                if (BVC_DBG(g, 16)) return;     // experiment: loads and barriers only
    #pragma unroll
                for (int i = 0; i < TM; ++i)
    #pragma unroll
                    for (int j = 0; j < TN; ++j)
                        // operands swapped: D = Bfrag^T-view x Afrag gives lane (l&15) = m, regs = 4 consecutive n
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
                if (do_rowsum) {
    #pragma unroll
                    for (int i = 0; i < TM; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[ks][i], accb[i], 0, 0, 0);
                }
            };
            mfma_half(0);   // needs only the first half's fragments: the second half's LDS reads retire underneath
            if (it + 2 < nt) {
                // own fragment reads retired, then the barrier: every wave is done with this slot -> refill it
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (!BVC_DBG(g, 32)) stage_tile<BM, AT>(ra, m0, (t0 + it + 2) * BK, p.lda, slot, wave, lane);
                if (!BVC_DBG(g, 8 | 32)) stage_tile<BN, BT>(rb, n0, (t0 + it + 2) * BK, p.ldb, slot + A_BYTES, wave, lane);
            }
            mfma_half(1);
            if (it + 1 < nt) {
                // K-step it+1 must have landed everywhere before the next iteration reads it; the refill just issued may fly on
                if (it + 2 < nt && !BVC_DBG(g, 8 | 32)) wait_vmcnt<DMA_PER_STAGE>(); else wait_vmcnt<0>();
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS is reused by the epilogue
    // ------------------------------------------------------------------ epilogue
    // The MFMA fragment layout gives each lane 4 columns of one row: stored directly, a wave touches 16 rows x 32 B
    // per instruction and the write path reaches only ~2.2 TB/s (measured).  Instead every wave parks its f32 tile in
    // LDS (free after the K loop; XOR-swizzled 16-B units, no bank conflicts) and re-reads it row-major, so each lane
    // owns 8 consecutive columns and every global load / store of the epilogue is a full 128-B line per 8 lanes.
#ifdef BVC_BODY_GATE
    constexpr int epi = EPI_RESID_GATE;
#else
    const int epi = p.epi;
#endif
    const float alpha = p.alpha_dev ? p.alpha * p.alpha_dev[0] : p.alpha;
    float sumsq = 0.f, possum = 0.f;
    const bool atomic = p.split_k > 1;
    constexpr int UNITS = WN / 4;                       // 16-B units per tile row
    AS3 char* wl = (AS3 char*)smem + wave * (WM * WN * 4);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = 16 * i + (lane & 15);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int unit = (4 * j + (lane >> 4)) ^ (row & (UNITS - 1));
            *reinterpret_cast<AS3 f32x4*>(wl + row * (WN * 4) + unit * 16) = acc[i][j];
        }
    }
    if (atomic) {
        // split-K: f32 atomics straight into C.  Float atomics run at full rate only when a wave-instruction covers whole
        // contiguous rows (256 B = one row of a 64-wide wave tile, or two 128-B rows of a 32-wide one), so the lanes walk
        // the parked tile one dword each, row by row, instead of the 8-column chunks of the store path.
        if (DET || nt > 0) {      // (deterministic: every split writes its slab, an empty K range as zeros)
            float* cbase = reinterpret_cast<float*>(p.C);
#pragma unroll 4
            for (int idx = lane; idx < WM * WN; idx += 64) {
                const int row = idx / WN, col = idx % WN;
                const int m = m0 + wm * WM + row, n = n0 + wn * WN + col;
                const int unit = (col >> 2) ^ (row & (UNITS - 1));
                float v = *reinterpret_cast<const AS3 float*>(wl + row * (WN * 4) + unit * 16 + (col & 3) * 4) * alpha;
                if (m < p.M && n < p.N) {
                    if (p.bias && split == 0) v += p.bias[n];
                    if constexpr (DET) p.partial[((size_t)split * p.M + m) * p.N + n] = v;
                    else atomicAdd(cbase + (size_t)m * p.ldc + n, v);
                }
            }
        }
    } else if (nt > 0 || !atomic) {
        constexpr int CPR = WN / 8;                     // 8-column chunks per row
        constexpr int NCH = WM * WN / 8 / 64;           // chunks per lane
        // Chunk `it` of a lane is row it * (64 / CPR) + lane / CPR, columns 8 (lane % CPR) .. +7: the columns never change.
        const int cc = lane % CPR, rsub = lane / CPR;
        const int n = n0 + wn * WN + cc * 8;
        const bool ncol_ok = n < p.N;
        // On gfx950 loads and stores retire through ONE in-order counter (vmcnt): a load issued after a store cannot be
        // waited for without waiting for that store's write acknowledgement too.  The epilogue used to alternate
        // "load side input, compute, store" per chunk and so paid one store round trip per chunk - measured as ~5 us of fixed
        // cost per tile (tools/ab/gemm_dbg.py: decoder fc1 340 us, 201 us with the stores dropped).  All side inputs of the tile
        // (bias, residual, GELU' argument, labels, positional rows) are therefore fetched FIRST, into registers the parked
        // accumulators no longer need, and the stores follow back to back.
        f32x4 bias0 = {0.f, 0.f, 0.f, 0.f}, bias1 = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && (!atomic || split == 0) && ncol_ok) {
            bias0 = *reinterpret_cast<const f32x4*>(p.bias + n);
            bias1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
        }
        f32x4 side0[NCH], side1[NCH];     // f32 addend (residual / positional row / labels) or the 4 dwords of the bf16 aux row
        const bool side_f32 = (BVC_IS_RESID(epi) && !atomic) || epi == EPI_POS || epi == EPI_E2D || epi == EPI_LOSS;
        const bool side_aux = epi == EPI_DGELU || epi == EPI_DRELU;
        if (side_f32 || side_aux) {
#pragma unroll
            for (int it = 0; it < NCH; ++it) {
                const int m = m0 + wm * WM + it * (64 / CPR) + rsub;
                side0[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                side1[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (m >= p.M || !ncol_ok) continue;
                if (side_aux) {
                    side0[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const bf16_t*>(p.aux) + (size_t)m * p.ldaux + n);
                } else {
                    const float* src = BVC_IS_RESID(epi) ? p.resid + (size_t)m * p.ldc + n
                                     : epi == EPI_LOSS  ? p.labels + (size_t)m * p.ldc + n
                                                        : p.pos + (size_t)p.rowtok[m] * p.N + n;
                    side0[it] = *reinterpret_cast<const f32x4*>(src);
                    side1[it] = *reinterpret_cast<const f32x4*>(src + 4);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NCH; ++it) {
            const int row = it * (64 / CPR) + rsub;
            const int m = m0 + wm * WM + row;
            const f32x4 lo = *reinterpret_cast<const AS3 f32x4*>(wl + row * (WN * 4) + (((2 * cc) ^ (row & (UNITS - 1))) << 4));
            const f32x4 hi = *reinterpret_cast<const AS3 f32x4*>(wl + row * (WN * 4) + (((2 * cc + 1) ^ (row & (UNITS - 1))) << 4));
            if (m >= p.M || !ncol_ok) continue;
            float v[8] = {lo[0] * alpha + bias0[0], lo[1] * alpha + bias0[1], lo[2] * alpha + bias0[2], lo[3] * alpha + bias0[3],
                          hi[0] * alpha + bias1[0], hi[1] * alpha + bias1[1], hi[2] * alpha + bias1[2], hi[3] * alpha + bias1[3]};
            const size_t idx = (size_t)m * p.ldc + n;
            auto store_f32 = [&](float* dst) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
            };
            auto store_bf16 = [&](void* base, size_t at, const float* w) {
                if (BVC_DBG(g, 1)) return;
                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(base) + at) =
                    uint4{pack2bf(w[0], w[1]), pack2bf(w[2], w[3]), pack2bf(w[4], w[5]), pack2bf(w[6], w[7])};
            };
            auto add_side = [&]() {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] += side0[it][e]; v[4 + e] += side1[it][e]; }
            };
            switch (epi) {
                case EPI_F32: {
                    float* c = reinterpret_cast<float*>(p.C) + idx;
                    if (!DET && atomic) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) atomicAdd(c + e, v[e]);
                    } else {
                        store_f32(c);
                    }
                } break;
                case EPI_BF16: store_bf16(p.C, idx, v); break;
                case EPI_GELU: {
                    float a[8];
                    gelu_split(v, a);              // v <- gelu'(pre), a <- gelu(pre)
                    store_bf16(p.C, idx, v);
                    store_bf16(p.C2, idx, a);
                } break;
                case EPI_RESID: {
                    float* c = reinterpret_cast<float*>(p.C) + idx;
                    if (!DET && atomic) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) atomicAdd(c + e, v[e]);
                    } else {
                        add_side();
                        store_f32(c);
                    }
                } break;
                case EPI_POS: {
                    add_side();
                    store_f32(reinterpret_cast<float*>(p.C) + idx);
                } break;
                case EPI_E2D: {
                    add_side();
                    const size_t orow = (size_t)(m / p.rin) * p.rout + (m % p.rin);
                    store_f32(reinterpret_cast<float*>(p.C) + orow * p.ldc + n);
                } break;
                case EPI_LOSS: {
                    if (p.C2) store_f32(reinterpret_cast<float*>(p.C2) + idx);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] -= side0[it][e]; v[4 + e] -= side1[it][e]; }
#pragma unroll
                    for (int e = 0; e < 8; ++e) sumsq += v[e] * v[e];
                    store_bf16(p.C, idx, v);
                } break;
                case EPI_DGELU: {
                    const uint32_t w[4] = {__float_as_uint(side0[it][0]), __float_as_uint(side0[it][1]), __float_as_uint(side0[it][2]),
                                           __float_as_uint(side0[it][3])};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {      // aux = gelu'(pre), saved by the forward epilogue
                        v[2 * e] *= __uint_as_float(w[e] << 16);
                        v[2 * e + 1] *= __uint_as_float(w[e] & 0xffff0000u);
                    }
                    store_bf16(p.C, idx, v);
                } break;
                case EPI_F32_BF16: {
                    store_f32(reinterpret_cast<float*>(p.C) + idx);
                    store_bf16(p.C2, idx, v);
                } break;
                case EPI_RELU: {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                    store_bf16(p.C, idx, v);
                } break;
                case EPI_DRELU: {   // aux = the forward ReLU output: gradient passes where it was positive
                    const uint32_t w[4] = {__float_as_uint(side0[it][0]), __float_as_uint(side0[it][1]), __float_as_uint(side0[it][2]),
                                           __float_as_uint(side0[it][3])};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!((w[e] & 0x7fffu) && !(w[e] & 0x8000u))) v[2 * e] = 0.f;
                        if (!((w[e] & 0x7fff0000u) && !(w[e] & 0x80000000u))) v[2 * e + 1] = 0.f;
                    }
                    store_bf16(p.C, idx, v);
                } break;
                case EPI_NCE: {     // v = cos/T (alpha = 1/T): partial sums of exp(v - 1/T) over negatives and of v over positives
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int dj = n + e - m;
                        if (dj == 1 || dj == -1) possum += v[e];
                        else if (dj != 0) sumsq += __expf(v[e] - alpha);
                    }
                } break;
                case EPI_NCE_BWD: { // labels = {lse, pos_coef}: C bf16 = d loss / d v
                    const float lse = p.labels[0], pc = p.labels[1];
                    float w[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int dj = n + e - m;
                        w[e] = dj == 0 ? 0.f : (dj == 1 || dj == -1) ? pc : __expf(v[e] - lse);
                    }
                    store_bf16(p.C, idx, w);
                } break;
#ifdef BVC_BODY_GATE
                case EPI_RESID_GATE: {   // C f32 = resid + gate .* (v + bias): the gate multiplies the branch before the residual is added
                    const uint64_t q = ((uint64_t)m * p.N + n) >> 2;
                    const f32x4 g0 = gate_apply4(gate, m, q, f32x4{v[0], v[1], v[2], v[3]});
                    const f32x4 g1 = gate_apply4(gate, m, q + 1, f32x4{v[4], v[5], v[6], v[7]});
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] = g0[e]; v[4 + e] = g1[e]; }
                    add_side();
                    store_f32(reinterpret_cast<float*>(p.C) + idx);
                } break;
#endif
                default: break;
            }
        }
    }
    if (do_rowsum && (DET || nt > 0) && (lane >> 4) == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * WM + 16 * i + lane;
            if constexpr (DET) {
                if (m < p.M) p.ln_part[(size_t)split * p.M + m] = accb[i][0] * alpha;
            } else {
                if (m < p.M) atomicAdd(p.rowsum + m, accb[i][0] * alpha);
            }
        }
    }
    if (epi == EPI_NCE) {    // two partials per tile: [2 tile] = sum over negatives, [2 tile + 1] = sum over positives
        float* red = reinterpret_cast<float*>(smem);
        const float w0 = wave_sum(sumsq), w1 = wave_sum(possum);
        __syncthreads();
        if (lane == 0) { red[wave] = w0; red[4 + wave] = w1; }
        __syncthreads();
        if (tid == 0) {
            p.partial[2 * tile] = (red[0] + red[1]) + (red[2] + red[3]);
            p.partial[2 * tile + 1] = (red[4] + red[5]) + (red[6] + red[7]);
        }
    }
    if (epi == EPI_LOSS) {   // uniform per workgroup: deterministic per-tile partial of sum (logit-label)^2
        float* red = reinterpret_cast<float*>(smem);
        const float w = wave_sum(sumsq);
        __syncthreads();   // every wave is done with its tile in LDS
        if (lane == 0) red[wave] = w;
        __syncthreads();
        if (tid == 0) p.partial[tile] = (red[0] + red[1]) + (red[2] + red[3]);
    }
#undef BVC_IS_RESID
